// render_views.hip — many cameras of one scene in one wavefront batch (include/jsrt_views.h).
//
// A view's pixel stands where a caller's ray stands in a feed frame (render.hip color_frame): item i = v * W * H + p of
// the feed is pixel p of view v, and its level-0 ray is computed on the device from that view's camera (k_gen_views,
// in k_gen_rays's place).  Everything after level 0 -- the level loop, the pools, the two streams, the learned bounds,
// the redo of a poisoned frame -- is the feed frame's, unchanged.  k_store_colors leaves each (item, sample) colour in
// a staging buffer, and k_fold_views folds a pixel's samples, in sample order, with k_accum's arithmetic and
// k_final's finish.  View v is therefore, bit for bit, the frame render_frame gives a scene whose camera is cams[v].
#include "render_levels.h"

namespace jsrt {

// Level 0 of a view batch.  Path q of the batch is item W.p0 + q / nb, sample W.s0 + q % nb (k_gen_rays's order); the
// item's view and pixel follow from the feed's first item.  The key is k_gen's -- (seed of the view, pixel, sample),
// the view index is no part of it -- and so are the pre-root frame's draws: the jitter of the sampling renderers,
// then camera_ray's depth of field.  A wave's items almost always share a view (its camera is then one cached
// 168-byte record for the whole wave), but a wave may straddle two views, so each lane reads its own.
// Level counts as k_gen writes them; A.max_depth >= 1 (views_frame answers depth 0 itself).
__global__ __launch_bounds__(256) void k_gen_views(RenderArgs A, WArgs W, RayFeed F) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if ((!W.chain || W.hybrid) && q < LVL_UNDER) W.lvl[q] = q == 0 ? W.npaths : 0u;
    if (q >= W.npaths) return;
    const uint32_t nb = W.npaths / W.npix;
    const uint32_t i = F.item0 + W.p0 + q / nb, smp = F.sample0 + W.s0 + q % nb;
    const uint32_t v = i / F.view_px, pixel = i - v * F.view_px;  // (v < F.nviews: the feed ends with the last view)
    if (!W.chain) {
        W.path[q] = q;
        W.parent[q] = NO_PARENT;
    }
    const int py = (int)(pixel / (uint32_t)A.W), px = (int)(pixel % (uint32_t)A.W);
    const uint32_t key = mix32(mix32(F.seeds ? F.seeds[v] : A.seed, pixel), smp);
    Rng pre{key, 0u, 0u};  // pre-root frame (address 0): jitter, then DOF draws
    double x = 2 * ((double)px / A.W) - 1, y = -2 * ((double)py / A.H) + 1;  // renderers.js:22-25
    if (A.kind != JSRT_RENDERER_SIMPLE) {
        const double jx = x + (2.0 / A.W) * (pre.next() - 0.5);  // renderers.js:95-96
        const double jy = y + (2.0 / A.H) * (pre.next() - 0.5);
        x = jx;
        y = jy;
    }
    F3 o, d;
    camera_ray(F.cams[v], x, y, pre, o, d);
    W.ox[q] = o.x; W.oy[q] = o.y; W.oz[q] = o.z;
    W.dx[q] = d.x; W.dy[q] = d.y; W.dz[q] = d.z;
    W.addr[q] = mix32(0u, 1u);
    W.key[q] = key;
    W.prim[q] = -1;
}

// What k_fold_views folds: samples [s0, s0 + ns) of items [item0, item0 + n) of the views' pixels, staged by
// k_store_colors as stage[3 * (i * ns + s)] (null: every colour black, World.color(ray, 0)).  acc (n x 4 f32, nullable
// when one chunk holds every sample) carries an item's accumulator from one chunk of samples to the next.
struct ViewFold {
    const float *stage;
    float *acc;
    uint32_t item0, n, s0, ns;
};

// One lane per (view, pixel): the chunk's samples of the pixel into its accumulator in sample order, with k_accum's
// arithmetic (render_levels.h accumulate: Incremental the f32 sum, RandomMultisampling the sum of sample / spp, Simple
// the sample); after the pixel's last sample k_final's finish -- times(1 / passes) for the Incremental renderer, then
// PixelBuffer.setColor -- into pixel py * W + px of its view, row-major.
__global__ __launch_bounds__(256) void k_fold_views(RenderArgs A, ViewFold V) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= V.n) return;
    F3 acc = f3(0, 0, 0);
    if (V.s0 > 0) acc = f3(V.acc[4 * (size_t)t], V.acc[4 * (size_t)t + 1], V.acc[4 * (size_t)t + 2]);
    const float *c = V.stage ? V.stage + 3 * (size_t)t * V.ns : nullptr;
    for (uint32_t s = 0; s < V.ns; ++s) acc = accumulate(A, acc, c ? f3(c[3 * s], c[3 * s + 1], c[3 * s + 2]) : f3(0, 0, 0));
    if (V.s0 + V.ns < (uint32_t)A.spp) {
        V.acc[4 * (size_t)t] = acc.x;
        V.acc[4 * (size_t)t + 1] = acc.y;
        V.acc[4 * (size_t)t + 2] = acc.z;
        return;
    }
    const F3 out = (A.kind == JSRT_RENDERER_INCREMENTAL) ? scale(acc, 1.0 / (int32_t)A.spp) : acc;  // times(1/(iter+1))
    const size_t p = (size_t)V.item0 + t;
    A.rgba[p] = set_color_rgba(out);
    if (A.colors) {
        A.colors[4 * p] = out.x;
        A.colors[4 * p + 1] = out.y;
        A.colors[4 * p + 2] = out.z;
        A.colors[4 * p + 3] = 1.0f;
    }
}

// The chunks of a view frame: the nviews x W x H items in ranges of at most max_paths (whole 64s, so a range may
// start and end in the middle of a view), and a range's samples in chunks of as many as max_paths holds.  Each chunk
// is one feed frame into the staging buffer (<= max_paths x 12 B) and one fold; a range's accumulators persist across
// its chunks (and are not needed when one chunk holds every sample).
hipError_t views_frame(const DScene &S, const RenderArgs &A, const RayFeed &F, int ns, Wavefront &wf, hipStream_t st,
                       KernelTimes *kt, size_t max_paths) {
    if (!F.cams || F.nviews == 0 || !A.rgba || A.W <= 0 || A.H <= 0 || A.spp <= 0 || A.max_depth < 0 ||
        A.max_depth > MAX_TREE_DEPTH)
        return hipErrorInvalidValue;
    const uint64_t total = (uint64_t)F.nviews * (uint64_t)A.W * (uint64_t)A.H;
    if (total >= ((uint64_t)1 << 31)) return hipErrorInvalidValue;
    const uint32_t N = (uint32_t)total, spp = (uint32_t)A.spp;
    auto fold = [&](const ViewFold &V) {
        const bool ev = kt && kt->on(KT_FINAL);
        if (ev) kt->ev[KT_FINAL].begin(st);
        hipLaunchKernelGGL(k_fold_views, dim3(grid(V.n)), dim3(256), 0, st, A, V);
        if (ev) kt->ev[KT_FINAL].end(st);
        return hipGetLastError();
    };
    if (A.max_depth == 0)  // World.color(ray, 0) = black (world.js:32): nothing is traced
        return fold(ViewFold{nullptr, nullptr, 0u, N, 0u, spp});
    const size_t cap = std::max<size_t>(64, max_paths);
    const uint32_t ci = (size_t)N <= cap ? N : (uint32_t)std::min<size_t>(cap & ~(size_t)63, (size_t)1 << 30);
    const uint32_t cs = (uint32_t)std::max<size_t>(1, std::min<size_t>(cap / ci, spp));
    float *stage = nullptr, *acc = nullptr;
    hipError_t e = hipMallocAsync((void **)&stage, (size_t)ci * cs * 3 * sizeof(float), st);
    if (e == hipSuccess && cs < spp) e = hipMallocAsync((void **)&acc, (size_t)ci * 4 * sizeof(float), st);
    for (uint32_t i0 = 0; i0 < N && e == hipSuccess; i0 += ci) {
        const uint32_t n = std::min(ci, N - i0);
        for (uint32_t s0 = 0; s0 < spp && e == hipSuccess; s0 += cs) {
            const uint32_t nsmp = std::min(cs, spp - s0);
            RayFeed C{};
            C.out = stage;
            C.n = n;
            C.spp = nsmp;
            C.sample0 = s0;
            C.cams = F.cams;
            C.seeds = F.seeds;
            C.nviews = F.nviews;
            C.view_px = (uint32_t)A.W * (uint32_t)A.H;
            C.item0 = i0;
            // (a feed frame returns with its batches done and clean: a poisoned one was redone, staging and all)
            if ((e = color_frame(S, A, C, ns, wf, st, kt, max_paths)) != hipSuccess) break;
            e = fold(ViewFold{stage, acc, i0, n, s0, nsmp});
        }
    }
    if (stage) (void)hipFreeAsync(stage, st);
    if (acc) (void)hipFreeAsync(acc, st);
    return e;
}

}  // namespace jsrt
