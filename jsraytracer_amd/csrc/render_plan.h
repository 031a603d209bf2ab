// render_plan.h — the host arithmetic of a frame (render.hip run_frame), which the driver only plumbs:
//   * the run-time knobs (FrameKnobs), the shape of the batches (plan_batches), their enumeration (batch_span,
//     two_full) and the pixel order inside them (pixel_of);
//   * the schedule (schedule_of) and, per attempt, the size of a batch pool (initial_pool_factor, pool_shape), the
//     per-level launch bounds (level_bounds) and the schedule words of a WArgs (batch_settings);
//   * what a scene learns from its frames (LearnedPool: learn_fractions, redo_step after a poisoned frame);
//   * the layout of a batch pool, stated once (pool_fields) and visited by a sizer (pool_bytes) and a carver
//     (carve_pool), with fix_capacity and the per-path estimate that caps the default batch (pool_bytes_per_path).
// No HIP calls and no getenv: the header builds for the host alone (tests/native/batch_plan_host.hip with
// tests/test_batch_plan.py, tests/native/frame_policy_host.hip with tests/test_frame_policy.py).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <type_traits>

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

// The schedule of a scene's frames: chain when no node can have two children; otherwise the hybrid chain
// (side chains for second children) for flat scenes, the tree for BVH / SDF scenes (JSRT_HYBRID=0/1 forces
// one).  A/B on MI355X (profiles/r04_s6_ab.txt): cornell hybrid 493.8 vs tree 466.3 Ms/s; bunny 518.4 vs
// 555.7, dragon 785.4 vs 792.5, SDF_Menger 112.8 vs 116.1 -- the tree's octant-sorted appends keep BVH
// casts coherent, and its compaction suits sky-heavy scenes.
inline int schedule_of(const DScene &S, const FrameKnobs &K) {
    if (S.max_children <= 1) return SCHED_CHAIN;
    if (K.hybrid >= 0) return K.hybrid ? SCHED_HYBRID : SCHED_TREE;
    return S.profile == PF_ANALYTIC ? SCHED_HYBRID : SCHED_TREE;
}
constexpr size_t HYBRID_POOL_FACTOR = 2;  // initial hybrid side-chain slots: paths x factor / 4

// The first pool of a batch shape (tree / hybrid chain): a batch of at most 1 M paths starts with 3 side-chain
// slots per path (a band of columns through a glass sphere outgrows the default 0.5 -- a redo the memory of small
// batches need not risk)
inline size_t initial_pool_factor(int sched, size_t paths, const FrameKnobs &K) {
    if (K.pool_factor) return K.pool_factor;
    return sched == SCHED_HYBRID ? (paths <= ((size_t)1 << 20) ? 8 : HYBRID_POOL_FACTOR) : 8;
}

// What Wavefront::reserve lays out.  rays: ray slots; nodes: node records; hands: hand-off records; paths: root
// colours; mode: SCHED_*; shadow: light-sample entries of the persistent shadow casts (0 if unused)
struct PoolDims {
    size_t rays, nodes, hands, paths;
    int mode;
    size_t shadow;
};
// A batch pool for `paths` paths at one pool factor.  fits: the hybrid chain's u32 node index holds cap x depth.
struct PoolShape {
    size_t cap;        // chain slots per level (hybrid: paths + side chains, 256-aligned)
    size_t pool, level_cap;
    int group;         // WArgs::group
    size_t hands, shadow;
    bool fits;
    PoolDims dims;
};
inline PoolShape pool_shape(int sched, size_t paths, int depth, size_t pool_factor, int ns, bool persist,
                            const FrameKnobs &K) {
    const bool hybrid = sched == SCHED_HYBRID, chain = sched != SCHED_TREE;
    PoolShape P{};
    P.cap = hybrid ? ((paths + paths * pool_factor / 4 + 255) & ~(size_t)255) : paths;
    P.fits = !(hybrid && P.cap * (size_t)depth >= ((size_t)1 << 32));
    P.pool = chain ? P.cap : paths * pool_factor;
    P.level_cap = chain ? P.cap : P.pool / 2;
    // k_shadow: a node's light samples on `group` lanes (one each), or all on one lane (group 1: more than
    // 64 samples, or JSRT_SHADOW_SERIAL=1, an A/B knob)
    P.group = 1;
    if (ns > 1 && ns <= 64 && !(K.shadow_serial && !persist))
        while (P.group < ns) P.group *= 2;
    // hand-off slots: one per node of a level; level 0 holds all `paths` camera rays, the
    // deeper levels at most level_cap (k_shade poisons the batch before writing past it)
    P.hands = chain ? P.cap : std::max(P.level_cap, paths);
    P.shadow = persist ? P.hands * (size_t)P.group : 0;
    P.dims = chain ? PoolDims{P.cap, P.cap * (size_t)depth, P.cap, paths, sched, P.shadow}
                   : PoolDims{P.pool, P.pool, P.hands, paths, SCHED_TREE, P.shadow};
    return P;
}

// Per-level launch bound of a batch of np paths (run_batch's `bound`): the most the level can hold, or -- from
// learned level counts, unless the frame is a conservative redo -- frac[L] x np with JSRT_BOUND_MARGIN and slack.
inline std::vector<size_t> level_bounds(int sched, uint32_t np, const PoolShape &P, int max_depth, int max_children,
                                        const std::vector<double> &frac, bool conservative, const FrameKnobs &K) {
    std::vector<size_t> b(std::max(1, max_depth), 0);
    auto learned = [&](int L, size_t most) {
        return std::min(most, std::max<size_t>(256, (size_t)((double)np * frac[L] * K.bound_margin) + K.bound_slack));
    };
    if (sched == SCHED_HYBRID) {  // level L: its live chains (<= cap)
        for (int L = 0; L < max_depth; ++L) {
            b[L] = L == 0 ? np : P.cap;
            // (at least one block: a launch that can set LVL_UNDER for every level chains may continue into, even
            // at a learned count of 0)
            if (L > 0 && !conservative && L < (int)frac.size()) b[L] = learned(L, P.cap);
        }
        return b;
    }
    size_t ub = np;
    for (int L = 0; L < max_depth && ub > 0; ++L) {
        b[L] = ub;
        if (!conservative && L < (int)frac.size()) b[L] = learned(L, ub);
        ub = L + 1 < max_depth ? std::min(ub * (size_t)max_children, P.level_cap) : 0;
    }
    return b;
}

// The frame's settings of a pool's WArgs: the schedule words.  Every pointer and stride stays the pool's.
inline void batch_settings(WArgs &W, const DScene &S, const FrameKnobs &K, const BatchPlan &plan, const PoolShape &P,
                           int ns, int sched) {
    const bool chain = sched != SCHED_TREE;
    W.ns = ns;
    W.group = P.group;
    // the node-per-lane k_shadow_node where run_batch's conditions hold (one area light of 2..4 samples in a
    // flat scene); JSRT_SHADOW_NODE=0/1 forces the lane-per-sample k_shadow / asks for the node form
    W.shadow_node = K.shadow_node ? 1 : 0;
    W.chain = chain ? 1 : 0;
    W.hybrid = sched == SCHED_HYBRID ? 1 : 0;
    W.cap = (uint32_t)P.cap;
    // shadow hand-off bucketed by hit primitive (<= BKT_N buckets of consecutive primitives)
    int shift = 0;
    while (S.n_prims > 0 && ((S.n_prims - 1) >> shift) >= BKT_N) ++shift;
    W.bucket = (sched != SCHED_CHAIN && !plan.persist && S.n_prims > 0 && ns > 0 && ns <= 64 && K.bucket) ? shift + 1 : 0;
    W.pool = P.pool;
    W.level_cap = P.level_cap;
    // children grouped by direction octant where the next cast walks a BVH (A/B on MI355X,
    // profiles/r03_s3_ab.txt: bunny +5.5 %; cornell -0.8 %, its keyed append costing k_shade 3 ms)
    W.child_sort = !chain && (K.child_sort >= 0 ? K.child_sort == 1 : ((S.profile & PF_BVH) != 0));  // (tree appends only)
    // hand-off buckets keyed by the hit point's grid cell, with per-cell shadow-root masks, for flat
    // scenes (cornell +1.5 %, r03_s15); by hit primitive (runs of consecutive triangles) for meshes,
    // where the BVH and not the root loop carries the shadow casts (bunny +-0.2 %, r03_s6)
    const bool grid = K.bucket_grid >= 0 ? K.bucket_grid == 1 : S.profile == PF_ANALYTIC;
    W.bucket_grid = (W.bucket && S.grid_cells > 0 && grid) ? 1 : 0;
    W.pixel_major = plan.pixel_major ? 1 : 0;  // the order of a batch's paths (plan_batches)
}

// Learn the level counts from a batch's read-back lvl words (clean batches only), as the maximum over the batches
// seen: level L's rays (hybrid: chains continuing into L + side chains started at L) per path of the batch.
inline void learn_fractions(std::vector<double> &frac, const uint32_t *lvl, int max_depth, bool hybrid, uint32_t npaths) {
    if (lvl[LVL_FLAG] || lvl[LVL_UNDER]) return;
    if (frac.size() < (size_t)max_depth) frac.assign(max_depth, 0.0);
    for (int L = 0; L < max_depth; ++L)
        frac[L] = std::max(frac[L], (double)(hybrid ? lvl[2 * L] + lvl[2 * L + 1] : lvl[L]) / (double)npaths);
}

// What follows a poisoned frame (flag: a pool's LVL_FLAG, under: its LVL_UNDER; one of them set): the learned
// state for the redo, or no larger pool to redo it with.
enum class Redo { AGAIN, OUT_OF_MEMORY };
inline Redo redo_step(LearnedPool &st, bool *twin_fix_all, int sched, size_t paths, bool flag, bool under,
                      bool &conservative) {
    (void)under;
    if (sched == SCHED_CHAIN) {  // chain: only k_shade's k_fix_dirs records can run out (fix_record)
        // both pools take a record per ray slot (the overflow may have been in either); the setting stays for
        // later frames, like a doubled pool_factor.  A second overflow cannot happen: a level writes at most
        // one record per ray slot
        if (st.fix_all && (!twin_fix_all || *twin_fix_all)) return Redo::OUT_OF_MEMORY;
        st.fix_all = true;
        if (twin_fix_all) *twin_fix_all = true;
    } else if (flag) {  // a batch outgrew the pool: twice the pool, relearn the counts
        if (paths * st.pool_factor > ((size_t)1 << 31) * (sched == SCHED_HYBRID ? 4 : 1)) return Redo::OUT_OF_MEMORY;
        st.pool_factor *= 2;
        st.frac.clear();
    } else {  // a level outgrew its learned bound: redo with the conservative bounds (and relearn)
        conservative = true;
        st.frac.clear();
    }
    return Redo::AGAIN;
}

// k_fix_dirs records of a pool.  Unstable spherePicks per level: ~1e-5 of the nodes; every node under
// JSRT_FORCE_EXACT_PICK, or after a frame that ran out of records (fix_all: the frame is redone with one record
// per ray slot).  (JSRT_FIX_CAP=n, a test knob: n records until a frame runs out, to exercise the redo on either pool)
inline size_t fix_capacity(bool fix_all, size_t rays, const FrameKnobs &K) {
    return fix_all ? rays + 4096 : K.fix_cap >= 0 ? (size_t)K.fix_cap : K.force_exact_pick ? rays + 4096 : rays / 8 + 4096;
}

// The layout of a batch pool: f(field of w, elements) for every buffer the mode uses, in address order.  Each starts
// 256-aligned.  The one statement of the layout: pool_bytes sizes it and carve_pool assigns it.
template <class F>
inline void pool_fields(WArgs &w, const PoolDims &d, size_t fixcap, F &&f) {
    const bool tree = d.mode == SCHED_TREE, hybrid = d.mode == SCHED_HYBRID;
    f(w.ox, d.rays); f(w.oy, d.rays); f(w.oz, d.rays);
    f(w.dx, d.rays); f(w.dy, d.rays); f(w.dz, d.rays);
    f(w.addr, d.rays); f(w.key, d.rays);
    f(w.t, d.rays); f(w.prim, d.rays); f(w.ctx, d.rays);
    if (tree) f(w.path, d.rays);
    if (tree || hybrid) f(w.parent, d.rays);
    if (hybrid) { f(w.list0, d.rays); f(w.list1, d.rays); f(w.endl, d.rays); }  // live lists, last levels
    f(w.node, d.nodes);
    f(w.child, 4 * d.nodes);
    if (tree) f(w.slot, 2 * d.nodes);
    if (hybrid) f(w.slot, d.nodes);  // (second children)
    if (tree || hybrid) f(w.root, 3 * d.paths);
    f(w.hand, HAND_PLANES * d.hands);
    f(w.hnode, d.hands);
    f(w.lvl, 64);   // level counts and frame flags
    f(w.qctr, 64);  // work counters
    f(w.fixrec, 3 * fixcap);
    f(w.fixctr, 64);
    if (d.shadow) { f(w.sray, 2 * d.shadow); f(w.scol, d.shadow); }
    if (tree || hybrid) {  // buckets
        f(w.bkt, (size_t)MAX_TREE_DEPTH * BKT_LEVEL);
        f(w.bbase, (d.hands / 256 + 1) * BKT_N);
        f(w.brank, d.rays);
    }
}
inline size_t pool_bytes(const PoolDims &d, size_t fixcap) {
    WArgs w{};
    size_t bytes = 0;
    pool_fields(w, d, fixcap, [&](auto *&p, size_t n) { bytes += (n * sizeof(*p) + 255) & ~(size_t)255; });
    return bytes;
}
// w: every buffer of the layout from `base` on (pool_bytes(d, fixcap) bytes), the other pointers null, the strides
// and fixcap; the rest of w zero
inline void carve_pool(WArgs &w, const PoolDims &d, size_t fixcap, uint8_t *base) {
    w = WArgs{};
    pool_fields(w, d, fixcap, [&](auto *&p, size_t n) {
        p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(base);
        base += (n * sizeof(*p) + 255) & ~(size_t)255;
    });
    w.fixcap = (uint32_t)fixcap;
    w.nstride = d.nodes;
    w.hstride = d.hands;
    w.sstride = d.shadow;
}

// Device bytes of the batch state per path of a batch on schedule `sched`: an estimate of the layout above at the
// first pool of a large batch, which caps the default batch size (DESIGN.md §3 sets it beside the real figure).
inline size_t pool_bytes_per_path(const DScene &S, int ns, int max_depth, int sched) {
    const size_t ray = 8 * 4 + 8 + 2 * 4, node = 16 + 4 * 16, hand = HAND_PLANES * 16 + 4;
    const bool persist = (S.profile & PF_SDF) && S.all_roots_prims;
    size_t group = 1;
    while ((int)group < ns && ns <= 64) group *= 2;
    const size_t depth = (size_t)std::max(1, max_depth);
    if (sched == SCHED_CHAIN)  // chain: one ray and depth nodes per path
        return ray + depth * node + hand + (persist ? group * 48 : 0);
    if (sched == SCHED_HYBRID)  // per chain slot: ray + parent + rank, depth x (node + second-child slot), hand-off
        return (4 + HYBRID_POOL_FACTOR) * (ray + 17 + depth * (node + 16) + hand + (persist ? group * 48 : 0) +
                                           BKT_N * 4 / 256) / 4 + 12;
    const size_t pool = 8, level_cap = pool / 2;  // pool_shape: pool = 8 x paths, level_cap = pool / 2
    // + the bucketed hand-off's ranks (4 B per pool slot) and block bases (BKT_N words per 256 hand-off slots)
    return pool * (ray + 8 + node + 2 * 16 + 4) + level_cap * (hand + (persist ? group * 48 : 0) + BKT_N * 4 / 256) + 12;
}

}  // namespace jsrt
