// Host build of PositionalUVMaterial's mapping (jsraytracer_amd/csrc/posuv_map.h posuv_map, the function shade_node
// and k_material_uv call) for tests/test_posuv_map.py.
#include "../../jsraytracer_amd/csrc/posuv_map.h"

// rec: one PUVM record; pos: n x 4 f32 (material_data.position, w = 1); out: n x 2 f32
extern "C" void posuv_map_many(const jsrt_rec_posuv *rec, const float *pos, long n, float *out) {
    for (long i = 0; i < n; ++i) jsrt::posuv_map(*rec, pos[4 * i], pos[4 * i + 1], pos[4 * i + 2], out[2 * i], out[2 * i + 1]);
}
