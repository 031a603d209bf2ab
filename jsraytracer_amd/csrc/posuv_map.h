// posuv_map.h — PositionalUVMaterial.color's mapping (materials.js:188-191) operation by operation: the UV pair
// the wrapper writes into material_data before it delegates to its base material.  No HIP runtime calls, so the
// same code builds for the device (shade_node, k_material_uv) and for the host (tests/native/posuv_map_host.hip,
// tests/test_posuv_map.py).
//
//   delta   = origin.minus(data.position)                    Vec.map over origin's length: f32(origin[i] - position[i]),
//                                                            position = the world hit point with w = 1
//   data.UV = Vec.of(u_axis.dot(delta), v_axis.dot(delta))   Vec.dot over the AXIS's length (math.js:252-260): f64
//                                                            products summed left to right, one rounding to f32
//
// Built with -ffp-contract=off: every product and sum below is one IEEE operation, as in the reference.  The loader
// (scene_load.cpp) admits lengths 3 and 4 only, and no axis longer than origin (the reference would read
// delta[3] === undefined there: a NaN UV).
#pragma once
#include <stdint.h>

#include "../../include/jsrt_scene.h"

#ifndef JSRT_HD
#ifdef __HIPCC__
#define JSRT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define JSRT_HD inline
#endif
#endif

namespace jsrt {

JSRT_HD float posuv_dot(const float *axis, uint32_t len, float d0, float d1, float d2, float d3) {
    const double s = ((double)axis[0] * (double)d0 + (double)axis[1] * (double)d1) + (double)axis[2] * (double)d2;
    return (float)(len == 4u ? s + (double)axis[3] * (double)d3 : s);
}

// (px, py, pz): material_data.position (w = 1)
JSRT_HD void posuv_map(const jsrt_rec_posuv &m, float px, float py, float pz, float &u, float &v) {
    const float d0 = (float)((double)m.origin[0] - (double)px), d1 = (float)((double)m.origin[1] - (double)py),
                d2 = (float)((double)m.origin[2] - (double)pz);
    const float d3 = m.origin_len == 4u ? (float)((double)m.origin[3] - 1.0) : 0.0f;  // (read by 4-component axes only)
    u = posuv_dot(m.u_axis, m.u_len, d0, d1, d2, d3);
    v = posuv_dot(m.v_axis, m.v_len, d0, d1, d2, d3);
}

}  // namespace jsrt
