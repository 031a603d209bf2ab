// Host build of the texture sampler (jsraytracer_amd/csrc/texture_sample.h tex_sample, included by
// device_common.h) for tests/test_texture_sampler.py: TextureMaterialColor.color on the CPU.
#include "../../jsraytracer_amd/csrc/device_common.h"

// desc: {width, height, mode, clamp_u, clamp_v}; texels: width * height * 4 bytes (4-byte aligned); uv: n x 2 f32;
// out: n x 3 f32
extern "C" void tex_sample_many(const uint32_t *desc, const uint8_t *texels, const float *uv, long n, float *out) {
    jsrt_rec_texture T{};
    T.width = desc[0];
    T.height = desc[1];
    T.mode = desc[2];
    T.clamp_u = desc[3];
    T.clamp_v = desc[4];
    T.offset = 0;
    double q255[256];
    for (int b = 0; b < 256; ++b) q255[b] = (double)b / 255.0;  // as scene_load.cpp builds DScene::tex_q255
    for (long i = 0; i < n; ++i)
        jsrt::tex_sample(T, texels, q255, uv[2 * i], uv[2 * i + 1], out[3 * i], out[3 * i + 1], out[3 * i + 2]);
}
