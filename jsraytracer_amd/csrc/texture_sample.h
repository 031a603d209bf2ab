// texture_sample.h — TextureMaterialColor.color (materials.js:97-130) operation by operation in float64: the
// arithmetic of one texture look-up, with no HIP runtime calls, so the same code builds for the device (mc_eval,
// k_material_color) and for the host (tests/native/texture_sample_host.hip, tests/test_texture_sampler.py).
// device_common.h includes it after js_max / js_min (Math.max / Math.min), which it uses.
//
// Built with -ffp-contract=off: every product and sum below is one IEEE operation, as in the reference.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/jsrt_scene.h"

namespace jsrt {

// TextureMaterialColor.normalizeUV (materials.js:97-100); `%` is C fmod
JSRT_HD double tex_normalize(double c, bool clamp) {
    if (clamp) return js_min(js_max(c, 0.0), 1.0);  // Math.clamp (math.js:49-51): NaN propagates
    return fmod(fmod(c, 1.0) + 1.0, 1.0);
}

JSRT_HD double tex_round(double x) {  // Math.round (half toward +inf); the sign of a zero result is never read
    if (!__builtin_isfinite(x)) return x;
    double r = floor(x);
    if (x - r >= 0.5) r += 1.0;
    return r;
}

// Math.clamp(p, 0, n - 1) of a finite tap coordinate, as an index
JSRT_HD uint32_t tex_index(double p, uint32_t n) { return (uint32_t)js_min(js_max(p, 0.0), (double)(n - 1u)); }

// r, g, b of TextureMaterialColor.color({UV: [u, v]}) rounded to f32 once (Vec.from); the alpha the reference also
// sums is never read where the loader accepts a texture (scene_load.cpp).  q255: the 256 quotients byte / 255
// (correctly rounded float64, the reference's `data[i] / 255`; built on the host once per scene, DScene::tex_q255:
// a look-up instead of twelve f64 divisions per bilinear sample).  texels: the TEXL section (T.offset
// inside it, 4-byte aligned, width * height * 4 bytes: checked at load).  A UV that leaves a texel coordinate
// non-finite (NaN, or +-Infinity in wrap mode) reads `data[NaN]` in the reference: every channel NaN, and no index
// is formed here.
JSRT_HD void tex_sample(const jsrt_rec_texture &T, const uint8_t *texels, const double *q255, float u, float v,
                        float &r, float &g, float &b) {
    const double U = tex_normalize((double)u, T.clamp_u != 0), V = tex_normalize((double)v, T.clamp_v != 0);
    const double fx = U * (double)T.width - 0.5;
    const double fy = (1.0 - V) * (double)T.height - 0.5;
    if (!(__builtin_isfinite(fx) && __builtin_isfinite(fy))) {
        r = g = b = __builtin_nanf("");
        return;
    }
    const uint32_t *tx = reinterpret_cast<const uint32_t *>(texels + T.offset);
    double r0 = 0.0, r1 = 0.0, r2 = 0.0;
    auto tap = [&](double px, double bx, double py, double by) {  // materials.js:124-126
        const size_t index = (size_t)tex_index(py, T.height) * T.width + tex_index(px, T.width);
        const uint32_t t = tx[index];  // R | G << 8 | B << 16 | A << 24
        const double w = bx * by;
        r0 += w * q255[t & 0xFFu];
        r1 += w * q255[(t >> 8) & 0xFFu];
        r2 += w * q255[(t >> 16) & 0xFFu];
    };
    if (T.mode == JSRT_TEX_BILINEAR) {  // materials.js:109-113: `fx % 1` keeps the sign of fx; x outer, y inner
        const double mx = floor(fx), my = floor(fy), wx = fmod(fx, 1.0), wy = fmod(fy, 1.0);
        tap(mx, 1.0 - wx, my, 1.0 - wy);
        tap(mx, 1.0 - wx, my + 1.0, wy);
        tap(mx + 1.0, wx, my, 1.0 - wy);
        tap(mx + 1.0, wx, my + 1.0, wy);
    } else {  // "nearest" (materials.js:114-117): one tap of weight 1 x 1
        tap(tex_round(fx), 1.0, tex_round(fy), 1.0);
    }
    r = (float)r0;
    g = (float)r1;
    b = (float)r2;
}

}  // namespace jsrt
