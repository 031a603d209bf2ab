// render_plan.h — the host arithmetic of a frame's batches (render.hip render_frame): the run-time knobs, the
// shape of the batches, their enumeration, and the pixel order inside them.  No HIP calls: the header builds for
// the host alone (tests/native/batch_plan_host.hip, tests/test_batch_plan.py).
#pragma once
#include <stdint.h>

#include <algorithm>

#include "render_kernel.h"

namespace jsrt {

#ifndef TILE_PATCHES_DEFAULT
#define TILE_PATCHES_DEFAULT 8
#endif
#ifndef SPLIT_PIXELS_DEFAULT
#define SPLIT_PIXELS_DEFAULT true  // bunny 656.6 -> 687.2 M/s (profiles/r06_s9_bunny.txt)
#endif
// The run-time knobs of the render path (environment variables JSRT_<NAME>; A/B and test knobs), read once per
// frame by render.hip's frame_knobs(), the only getenv of the render path.  -1 = unset: the default is decided
// where the knob is used.
struct FrameKnobs {
    bool force_exact_pick = false;  // FORCE_EXACT_PICK=1 (tests): every diffuse pick through k_fix_dirs
    int fix_cap = -1;               // FIX_CAP=n (tests): n k_fix_dirs records until a frame runs out; default by pool
    int hybrid = -1;                // HYBRID=0/1: the tree / the hybrid chain for branching scenes; default by profile
    int pixel_major = -1;           // PIXEL_MAJOR=0/1: a pixel's samples side by side; default: not the analytic profile
    uint32_t batch_spp = 256;       // BATCH_SPP=n: samples of a pixel per pixel-major batch (>= 1)
    int tile_patches = TILE_PATCHES_DEFAULT;  // TILE_PATCHES=n: pixel-major pixels in tiles of n x n patches (0: raster)
    bool persist = true;            // PERSIST=0: no persistent casts for SDF scenes
    bool split_frame = true;        // SPLIT_FRAME=0: a frame that fits one batch stays one batch
    int split_min = 22;             // SPLIT_MIN=k: ... and is split from 2^k paths (1..40)
    bool split_pixels = SPLIT_PIXELS_DEFAULT;  // SPLIT_PIXELS=0/1: a pixel-major frame splits its pixels, not its samples
    size_t pool_factor = 0;         // POOL_FACTOR=n (tests): the first pool, >= 1; 0: default by schedule and batch
    double bound_margin = 1.25;     // BOUND_MARGIN=x (tests): learned launch bounds x this ...
    size_t bound_slack = 4096;      // ... + this many rays (0 when BOUND_MARGIN is set)
    int dual = -1;                  // DUAL=0/1: two batch pools on two streams; default: two comparable batches
    int split = -1;                 // SPLIT=0/1: k_shadow on a stream of its own; default: persistent casts, one pool
    bool shadow_serial = false;     // SHADOW_SERIAL=1: a node's light samples on one lane (not with persistent casts)
    bool shadow_node = true;        // SHADOW_NODE=0: never the node-per-lane k_shadow_node
    bool bucket = true;             // BUCKET=0: no bucketed shadow hand-off
    int child_sort = -1;            // CHILD_SORT=0/1: children grouped by direction octant; default: BVH profiles
    int bucket_grid = -1;           // BUCKET_GRID=0/1: buckets keyed by grid cell; default: the analytic profile
};

// The shape of a frame's batches: [p0, p0 + npix) pixels x [s0, s0 + nsb) samples each
struct BatchPlan {
    uint32_t npix, nsb;
    bool pixel_major;   // WArgs::pixel_major
    int tile_p;         // RenderArgs::tile_p
    bool persist;       // persistent casts (SDF scenes whose top level is primitives only)
    bool split_pixels;  // a split frame halves its pixels, not its samples
    bool split;         // a frame that fits one batch, cut into two halves for the two batch streams
};
inline BatchPlan plan_batches(const DScene &S, const RenderArgs &A, int ns, size_t max_paths, const FrameKnobs &K) {
    const uint32_t npix_total = (uint32_t)A.patches * 64u;
    if (ns > 4) max_paths = max_paths * 4 / (size_t)ns;  // the per-sample hand-off scales with ns
    if (max_paths < 64) max_paths = 64;
    uint32_t npix = npix_total, nsb = 1;  // batch: [p0, p0 + npix) pixels x [s0, s0 + nsb) samples
    if ((size_t)npix > max_paths) npix = (uint32_t)(max_paths & ~(size_t)63);
    else nsb = (uint32_t)std::max<size_t>(1, std::min<size_t>(max_paths / npix, (size_t)A.spp));
    if (A.samples_per_batch > 0) nsb = std::min<uint32_t>(nsb, (uint32_t)A.samples_per_batch);
    // Pixel-major batches (round 6; the BVH and SDF profiles, WArgs::pixel_major): a pixel's samples are side by
    // side in the batch, and a batch holds every sample of its pixels (up to JSRT_BATCH_SPP = 256) rather than a
    // few samples of every pixel.  The rays in flight (~0.5 M) then come from a small patch of the image, so their
    // casts walk a small part of the BVH and keep it in the caches.  The keyed RNG and the per-pixel
    // accumulation in sample order leave the image unchanged.  Measured (profiles/r06_s6_ab_pixel_major_*.txt,
    // r06_s7_dragon.txt, r06_s8_dragon.txt): bunny 556 -> 657 M/s, SDF_Menger 148 -> 160, the dragon 798 -> 889 in
    // pixel-major order alone, then 1,116 / 1,228 / 1,306 / 1,416 / 1,475 / 1,533 M/s at 8 / 16 / 32 / 64 / 128 /
    // 256 samples per batch; the flat hybrid chain loses (cornell k_accum's strided reads), so it keeps the
    // sample-major order.  JSRT_PIXEL_MAJOR=0/1: A/B.
    const bool pixel_major = K.pixel_major >= 0 ? K.pixel_major == 1 : S.profile != PF_ANALYTIC;
    if (pixel_major) {
        uint32_t want = std::min<uint32_t>(K.batch_spp, (uint32_t)A.spp);
        if (A.samples_per_batch > 0) want = std::min<uint32_t>(want, (uint32_t)A.samples_per_batch);
        if (nsb < want) {  // fewer pixels, more of their samples
            npix = (uint32_t)std::min<size_t>(npix_total, std::max<size_t>(64, (max_paths / want) & ~(size_t)63));
            nsb = (uint32_t)std::max<size_t>(1, std::min<size_t>(max_paths / npix, (size_t)want));
        }
    }
    // ... and their pixels in compact tiles of JSRT_TILE_PATCHES x JSRT_TILE_PATCHES 8 x 8 patches (pixel_of)
    const int tile_p = pixel_major ? K.tile_patches : 0;
    // persistent casts: SDF scenes whose top level is primitives only (JSRT_PERSIST=0 disables)
    const bool persist = (S.profile & PF_SDF) && S.all_roots_prims && K.persist;
    // A frame that fits one batch of 4 M paths or more (a rank's columns of a multi-GPU render) is cut into
    // two batches of half the samples, so that they run on the two batch streams (below).  Round 3 split only
    // from 32 M paths (cornell 1024^2 x 32 +3.6 %; halves of 16 M lost 5 %, profiles/r03_s18_ab.txt s28); with
    // the hybrid chain the halves win down to 4 M: cornell's 4-rank share (16.7 M paths) 32.0 -> 29.5 ms, its
    // 8-rank share (8.4 M) 17.0 -> 16.3 ms (tools/project_scaling.py, profiles/r05_s6_projection.txt).
    // JSRT_SPLIT_FRAME=0 keeps one batch; JSRT_SPLIT_MIN=k (A/B) splits from 2^k paths.
    // (Pixel-major batches split their pixels instead -- two halves of the image, every sample each -- so that the
    // rays in flight keep coming from few pixels; JSRT_SPLIT_PIXELS=0/1: A/B.)
    const bool split_pixels = pixel_major && K.split_pixels;
    bool split = false;
    if (!persist && K.split_frame && npix == npix_total && nsb == (uint32_t)A.spp && A.spp >= 2 &&
        (uint64_t)npix * (uint64_t)A.spp >= ((uint64_t)1 << K.split_min)) {
        split = true;
        if (split_pixels && npix_total >= 128) npix = ((npix_total / 2) + 63) & ~63u;  // whole patches: 64-pixel units
        else nsb = (uint32_t)((A.spp + 1) / 2);  // odd spp: halves of (spp + 1) / 2 and (spp - 1) / 2 samples
    }
    return BatchPlan{npix, nsb, pixel_major, tile_p, persist, split_pixels, split};
}

// The batches of a frame of npix_total pixels x spp samples: rows of nsb samples (the last one shorter), each cut
// into spans of npix pixels (the last one shorter), row by row -- a pixel's samples reach k_accum in order.
struct BatchSpan {
    uint32_t p0, npix, s0, nb;  // [p0, p0 + npix) pixels x [s0, s0 + nb) samples
};
inline uint32_t batch_rows(const BatchPlan &P, uint32_t spp) { return (spp + P.nsb - 1) / P.nsb; }
inline uint32_t batch_cols(const BatchPlan &P, uint32_t npix_total) { return (npix_total + P.npix - 1) / P.npix; }
inline BatchSpan batch_span(const BatchPlan &P, uint32_t npix_total, uint32_t spp, uint32_t row, uint32_t col) {
    const uint32_t s0 = row * P.nsb, p0 = col * P.npix;
    return BatchSpan{p0, std::min(P.npix, npix_total - p0), s0, std::min(P.nsb, spp - s0)};
}
// two streams need two batches of comparable size: a frame of one full batch and a small remainder
// (bunny: 32 M + 1.2 M paths) has nothing to overlap; the halves of a split frame do (odd spp: nsb and nsb - 1
// samples; pixels: patches that differ by one)
inline bool two_full(const BatchPlan &P, uint32_t npix_total, uint32_t spp) {
    return P.split || (uint64_t)npix_total * (uint64_t)spp >= 2 * (uint64_t)P.npix * P.nsb - (uint64_t)P.npix;
}

// patch-ordered owned pixel index -> (owned column c, row py, image column px).  8 x 8-pixel patches in raster order,
// or (A.tile_p > 0) in raster order within tiles of tile_p x tile_p patches taken in raster order, the last tile
// row and column partial: the pixels of consecutive indices, and so the rays a batch has in flight, then cover a
// compact region of the image rather than a band as wide as it (the BVH working set of their casts)
__host__ __device__ __forceinline__ bool pixel_of(const RenderArgs &A, uint32_t p, int &c, int &py, int &px) {
    int patch = (int)(p >> 6);
    const int lane = (int)(p & 63);
    if (A.tile_p > 0) {
        const int T = A.tile_p, pxn = A.patches_x, pyn = A.patches / A.patches_x;
        const int ty = patch / (pxn * T), r = patch - ty * pxn * T;  // (every tile row but the last is full)
        const int h = T < pyn - ty * T ? T : pyn - ty * T;
        const int tx = r / (T * h), r2 = r - tx * T * h;  // (every tile of the row but the last is full)
        const int w = T < pxn - tx * T ? T : pxn - tx * T;
        patch = (ty * T + r2 / w) * pxn + tx * T + r2 % w;
    }
    c = (patch % A.patches_x) * 8 + (lane & 7);
    py = (patch / A.patches_x) * 8 + (lane >> 3);
    if (c >= A.ncols || py >= A.H) return false;
    px = owned_to_px(c, A.x_offset, A.x_delt, A.col_block);
    return px < A.W;
}

}  // namespace jsrt
