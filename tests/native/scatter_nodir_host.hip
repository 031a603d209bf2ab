// Host build of the scatter of a Phong / Fresnel / path-tracing node (jsraytracer_amd/csrc/device_common.h
// scatter_children) for tests/test_scatter_last_level.py: the "children are not cast" form (NODIR, k_shade's last
// level) against the full one -- the child count and each child's col, w and k, bit for bit.
#include <string.h>

#include "../../jsraytracer_amd/csrc/device_common.h"

// Per hit, 24 doubles in: N (3, unit), R (3), refr (3), diff (3), spec (3), refl (3), trans (3), kr, has_refr,
// ray direction d (3) packed as the last three after key / addr / calls:
//   in[0..20] the seven vectors, in[21] kr, in[22] has_refr, in[23..25] d, in[26] key, in[27] addr, in[28] calls
// out: per hit 2 x 16 uint32 -- for the full form then NODIR: n, then ch0 {col, w, k lo, k hi}, ch1 {...}
constexpr int IN = 29, OUT = 17;
extern "C" void scatter_both(const double *in, long n, int mkind, double mirror_prob, int force_fix, unsigned *out,
                             unsigned *calls_out) {
    using namespace jsrt;
    for (long i = 0; i < n; ++i) {
        const double *x = in + IN * i;
        auto v = [&](int k) { return f3((float)x[3 * k], (float)x[3 * k + 1], (float)x[3 * k + 2]); };
        ShadeData sd{};
        sd.N = v(0);
        sd.R = v(1);
        sd.refr = v(2);
        sd.diff = v(3);
        sd.spec = v(4);
        sd.refl = v(5);
        sd.trans = v(6);
        sd.kr = x[21];
        sd.has_refr = x[22] != 0;
        const F3 d = f3((float)x[23], (float)x[24], (float)x[25]);
        for (int form = 0; form < 2; ++form) {
            Rng rng{(uint32_t)x[26], (uint32_t)x[27], (uint32_t)x[28]};
            Child c[2];
            memset(c, 0, sizeof c);
            uint32_t f0, f1;
            const int nc = form == 0 ? scatter_children<false>(mkind, mirror_prob, sd, d, rng, force_fix != 0, c[0], c[1], f0, f1)
                                     : scatter_children<true>(mkind, mirror_prob, sd, d, rng, force_fix != 0, c[0], c[1], f0, f1);
            unsigned *o = out + (2 * i + form) * OUT;
            o[0] = (unsigned)nc;
            for (int j = 0; j < 2; ++j) {
                unsigned *r = o + 1 + 8 * j;
                memset(r, 0, 8 * sizeof(unsigned));
                if (j >= nc) continue;  // (a slot without a child is unspecified in both forms)
                memcpy(r, &c[j].col, 12);
                memcpy(r + 3, &c[j].w, 12);
                memcpy(r + 6, &c[j].k, 8);
            }
            calls_out[2 * i + form] = rng.calls;
        }
    }
}
