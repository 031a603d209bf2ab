// render.hip — wavefront (breadth-first) evaluation of the reference's ray tree on MI355X.
//
// The reference evaluates World.color recursively, depth first (world.js:31-41 ->
// materials.js:271-333).  Two facts make a breadth-first schedule produce bit-identical results:
//   1. every random draw is keyed by the ray-tree address of its World.color frame
//      (DESIGN.md §2.3), never by global call order;
//   2. the only cross-node arithmetic is surface.plus(child.times(col).times(w).times(k)) in child
//      order, which k_reduce performs bottom-up with the same f32 roundings.
// So each kernel processes one bounce level of ALL paths of a batch:
//   k_gen      camera rays (renderers.js:95-96 jitter, cameras.js:29-52)                -> level 0
//   k_extend   closest hit per ray (World.cast, world.js:28-30), culled world loop
//   k_shade    Primitive.color + materialData + getBaseFactors + light samples + scatter;
//              children appended to the next level with wave-aggregated atomics
//   k_shadow   the shadow casts of a node's light samples + colorFromLights' sums
//   k_reduce   levels deepest -> 0: surface + children, into the parent's child slot
//   k_accum    per pixel, samples in order: the renderer's f32 accumulation
//   k_final    running mean + PixelBuffer.setColor rules -> RGBA8 (+ f32 colour)
// Every kernel is small and converged (all lanes run the same stage) with its own register
// budget; batches are (pixels x samples) with ray SoA buffers in HBM.
#include "render_levels.h"

#include <mutex>

namespace jsrt {

const char *const KT_NAMES[KT_N] = {"k_gen", "k_extend", "k_shade", "k_shadow", "k_reduce", "k_accum", "k_final",
                                    "k_resolve"};

// camera rays: one per path q of the batch, sample-major (neighbouring q are neighbouring pixels)
__global__ __launch_bounds__(256) void k_gen(DScene S, RenderArgs A, WArgs W) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if ((!W.chain || W.hybrid) && q < LVL_UNDER) W.lvl[q] = q == 0 ? W.npaths : 0u;  // level counts (not the frame flags)
    if (q >= W.npaths) return;
    int c = 0, py = 0, px = 0;
    const uint32_t nsb = W.npaths / W.npix;
    const uint32_t pl = W.pixel_major ? q / nsb : q % W.npix, sl = W.pixel_major ? q % nsb : q / W.npix;
    const uint32_t smp = W.s0 + sl;
    const bool valid = pixel_of(A, W.p0 + pl, c, py, px);
    if (!W.chain) {
        if (A.max_depth <= 0) {  // World.color(ray, 0) = black; no level is traced
            W.root[3 * q] = W.root[3 * q + 1] = W.root[3 * q + 2] = 0.0f;
            return;
        }
        W.path[q] = q;
        W.parent[q] = valid ? NO_PARENT : DEAD_RAY;
    }
    if (!valid || A.max_depth <= 0) {  // edge patch outside the image: no ray
        W.prim[q] = NO_RAY;
        return;
    }
    const uint32_t pixel = (uint32_t)(py * A.W + px);
    const uint32_t key = mix32(mix32(A.seed, pixel), smp);
    Rng pre{key, 0u, 0u};  // pre-root frame (address 0): jitter, then DOF draws
    double x = 2 * ((double)px / A.W) - 1, y = -2 * ((double)py / A.H) + 1;  // renderers.js:22-25
    if (A.kind != JSRT_RENDERER_SIMPLE) {
        const double jx = x + (2.0 / A.W) * (pre.next() - 0.5);  // renderers.js:95-96
        const double jy = y + (2.0 / A.H) * (pre.next() - 0.5);
        x = jx;
        y = jy;
    }
    F3 o, d;
    camera_ray(S.cam, x, y, pre, o, d);
    W.ox[q] = o.x; W.oy[q] = o.y; W.oz[q] = o.z;
    W.dx[q] = d.x; W.dy[q] = d.y; W.dz[q] = d.z;
    W.addr[q] = mix32(0u, 1u);
    W.key[q] = key;
    W.prim[q] = -1;
}

// The caller's rays in the camera's place (color_frame): path q of the batch is ray W.p0 + q / nb, sample W.s0 + q % nb:
// a ray's samples side by side, then the next ray's (the order k_gen calls pixel-major; at one sample per ray,
// neighbouring lanes shade neighbouring rays).  W.pixel_major is deliberately not read, here or in k_store_colors: it
// orders a frame's pixels for k_accum, and a ray batch has one order.  Keyed by (seed, the ray's key, sample).  The ray opens
// the root World.color frame, address mix32(0, 1): the pre-root frame's draws (jitter, DOF) belong to a camera.
// Level counts as k_gen writes them; A.max_depth >= 1 (color_frame answers World.color(ray, 0) itself).
__global__ __launch_bounds__(256) void k_gen_rays(RenderArgs A, WArgs W, RayFeed F) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if ((!W.chain || W.hybrid) && q < LVL_UNDER) W.lvl[q] = q == 0 ? W.npaths : 0u;
    if (q >= W.npaths) return;
    const uint32_t nb = W.npaths / W.npix;
    const uint32_t i = W.p0 + q / nb, smp = F.sample0 + W.s0 + q % nb;
    if (!W.chain) {
        W.path[q] = q;
        W.parent[q] = NO_PARENT;
    }
    const float *r = F.rays + 6 * (size_t)i;
    W.ox[q] = r[0]; W.oy[q] = r[1]; W.oz[q] = r[2];
    W.dx[q] = r[3]; W.dy[q] = r[4]; W.dz[q] = r[5];
    W.addr[q] = mix32(0u, 1u);
    W.key[q] = mix32(mix32(A.seed, F.keys ? F.keys[i] : i), smp);
    W.prim[q] = -1;
}

// tree schedule: surface + children, bottom-up into the parent's child slot (materials.js:277-330)
__global__ __launch_bounds__(256) void k_reduce(WArgs W, int L) {
    const LevelRange R = level_range(W, L);
    const uint32_t tt = blockIdx.x * 256 + threadIdx.x;
    if (tt >= R.count) return;
    const uint32_t i = R.base + tt;
    // the node record, its parent and its first child's colour and record are loaded together (most
    // nodes have exactly one child): one memory round trip instead of two dependent ones
    const float4 nd = W.node[i];
    const uint32_t p = W.parent[i];
    const float4 v0 = W.slot[i];
    const float4 c0 = W.child[i];
    const uint32_t info = f2u(nd.w);
    if (!(info & INFO_HIT) || p == DEAD_RAY) return;
    F3 c = f3(nd.x, nd.y, nd.z);
    const int n = (int)((info >> INFO_NCHILD_SHIFT) & 3);
    if (n > 0) c = add_child(W, i, 0u, c, f3(v0.x, v0.y, v0.z), info, &c0);
    if (n > 1) {
        const float4 v1 = W.slot[W.nstride + i];
        c = add_child(W, i, 1u, c, f3(v1.x, v1.y, v1.z), info);
    }
    if (p == NO_PARENT) {  // write_result
        float *dst = W.root + 3 * (size_t)W.path[i];
        dst[0] = c.x;
        dst[1] = c.y;
        dst[2] = c.z;
    } else {
        W.slot[(size_t)(p & 1u) * W.nstride + (p >> 1)] = make_float4(c.x, c.y, c.z, 0.0f);
    }
}

__global__ __launch_bounds__(256) void k_bucket_offsets(WArgs W, int L) {
    __shared__ uint32_t part[256];
    uint32_t *B = W.bkt + (size_t)L * BKT_LEVEL;
    constexpr int PER = BKT_K / 256;
    const int t = (int)threadIdx.x;
    uint32_t c[PER], sum = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) { c[j] = B[t * PER + j]; sum += c[j]; }
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {  // inclusive scan of the per-thread sums
        const uint32_t v = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t off = part[t] - sum;
#pragma unroll
    for (int j = 0; j < PER; ++j) { B[2 * BKT_K + t * PER + j] = off; off += c[j]; }
    if (t == 255) B[3 * BKT_K] = part[255];
}

// tree schedule: per pixel, the batch's samples in order
__global__ __launch_bounds__(256) void k_accum(RenderArgs A, WArgs W) {
    const uint32_t pl = blockIdx.x * 256 + threadIdx.x;
    if (pl >= W.npix || W.lvl[LVL_FLAG]) return;  // a poisoned frame is redone by the host
    int c, py, px;
    if (!pixel_of(A, W.p0 + pl, c, py, px)) return;
    const size_t oi = (size_t)c * A.H + py;
    F3 acc = f3(A.accum[4 * oi], A.accum[4 * oi + 1], A.accum[4 * oi + 2]);
    const uint32_t nsb = W.npaths / W.npix;
    for (uint32_t sl = 0; sl < nsb; ++sl) {
        const uint32_t q = W.pixel_major ? pl * nsb + sl : sl * W.npix + pl;
        acc = accumulate(A, acc, f3(W.root[3 * q], W.root[3 * q + 1], W.root[3 * q + 2]));
    }
    A.accum[4 * oi] = acc.x;
    A.accum[4 * oi + 1] = acc.y;
    A.accum[4 * oi + 2] = acc.z;
}

// chain schedule: path q's colour, resolved bottom-up over its levels (surface + child contribution; a
// last-level child is black without a cast)
__device__ __forceinline__ F3 resolve_path(const RenderArgs &A, const WArgs &W, uint32_t q) {
    F3 v = f3(0, 0, 0);  // World.color(ray, 0) = black
    for (int L = A.max_depth - 1; L >= 0; --L) {
        const uint32_t i = (uint32_t)L * W.cap + q;
        const float4 nd = W.node[i];
        const uint32_t info = f2u(nd.w);
        if (info & INFO_MISS) {
            v = f3(nd.x, nd.y, nd.z);
        } else if (info & INFO_HIT) {
            F3 col = f3(nd.x, nd.y, nd.z);
            if ((info >> INFO_NCHILD_SHIFT) & 3) col = add_child(W, i, 0, col, L == A.max_depth - 1 ? f3(0, 0, 0) : v, info);
            v = col;
        }
    }
    return v;
}

// chain schedule: per pixel, its samples in order
__global__ __launch_bounds__(256) void k_resolve(RenderArgs A, WArgs W) {
    const uint32_t pl = blockIdx.x * 256 + threadIdx.x;
    if (pl >= W.npix) return;
    int c, py, px;
    if (!pixel_of(A, W.p0 + pl, c, py, px)) return;
    const size_t oi = (size_t)c * A.H + py;
    F3 acc = f3(A.accum[4 * oi], A.accum[4 * oi + 1], A.accum[4 * oi + 2]);
    const uint32_t nsb = W.npaths / W.npix;
    for (uint32_t sl = 0; sl < nsb; ++sl) {
        const uint32_t q = W.pixel_major ? pl * nsb + sl : sl * W.npix + pl;
        acc = accumulate(A, acc, resolve_path(A, W, q));
    }
    A.accum[4 * oi] = acc.x;
    A.accum[4 * oi + 1] = acc.y;
    A.accum[4 * oi + 2] = acc.z;
}

// hybrid chain: the colour of chain c, which starts at level s, bottom-up over its levels (surface + the
// first child's contribution -- the chain's own next level -- + the second child's, a side chain's colour
// in slot[i]; children of the last level are black without a cast), materials.js:277-330
__device__ __forceinline__ F3 resolve_chain(const RenderArgs &A, const WArgs &W, uint32_t c, int s) {
    F3 v = f3(0, 0, 0);
    const int end = W.endl[c];
    // the node records of the chain's levels, loaded before the bottom-up pass (their addresses do not
    // depend on it): up to 8 levels' loads in flight at once instead of one dependent round trip per level
    constexpr int PRE = 8;
    float4 pre[PRE];
#pragma unroll
    for (int k = 0; k < PRE; ++k)
        if (s + k <= end) pre[k] = W.node[(uint32_t)(s + k) * W.cap + c];
    for (int L = end; L >= s; --L) {
        const uint32_t i = (uint32_t)L * W.cap + c;
        float4 nd = L - s < PRE ? pre[0] : W.node[i];
#pragma unroll
        for (int k = 1; k < PRE; ++k)
            if (L - s == k) nd = pre[k];
        const uint32_t info = f2u(nd.w);
        if (info & INFO_MISS) {
            v = f3(nd.x, nd.y, nd.z);
        } else if (info & INFO_HIT) {
            const bool last = L == A.max_depth - 1;
            const int n = (int)((info >> INFO_NCHILD_SHIFT) & 3);
            F3 col = f3(nd.x, nd.y, nd.z);
            if (n > 0) col = add_child(W, i, 0, col, last ? f3(0, 0, 0) : v, info);
            if (n > 1) {
                const float4 v1 = last ? make_float4(0, 0, 0, 0) : W.slot[i];
                col = add_child(W, i, 1, col, f3(v1.x, v1.y, v1.z), info);
            }
            v = col;
        }
    }
    return v;
}

// hybrid chain: the side chains that start at level s (ids npaths + [side(< s), side(<= s))), into their
// parents' second-child slots.  Launched for s = depth - 1 .. 1, so a chain's own side chains are resolved
// first.
__global__ __launch_bounds__(256) void k_resolve_side(RenderArgs A, WArgs W, int s) {
    if (W.lvl[LVL_FLAG]) return;
    const uint32_t lo = side_base(W, s);
    const uint32_t c = lo + blockIdx.x * 256 + threadIdx.x;
    if (c >= lo + W.lvl[2 * s + 1]) return;
    const F3 v = resolve_chain(A, W, c, s);
    W.slot[W.parent[c]] = make_float4(v.x, v.y, v.z, 0.0f);
}

// hybrid chain: every path's colour -> root (k_accum adds them per pixel in sample order)
__global__ __launch_bounds__(256) void k_fix_dirs(WArgs W) {
    const uint32_t n = *W.fixctr, m = n < W.fixcap ? n : W.fixcap;
    // a child slot past the ray arrays belongs to a frame k_shade flagged for a redo (out of chain slots or
    // pool): not written
    const size_t bound = W.chain ? (size_t)W.cap : (size_t)W.pool;
    for (uint32_t k = threadIdx.x; k < m; k += 256) {
        const uint4 a = W.fixrec[3 * (size_t)k], b = W.fixrec[3 * (size_t)k + 1], c = W.fixrec[3 * (size_t)k + 2];
        const F3 N = f3(__uint_as_float(c.x), __uint_as_float(c.y), __uint_as_float(c.z));
        for (int j = 0; j < 2; ++j) {
            const uint32_t f = j == 0 ? b.x : b.y;
            if (j >= (int)b.z || f == 0u) continue;
            Rng rg{a.z, a.w, (f & 0x7FFFFFFFu) - 1u};  // the pick's draws (path_scatter: theta, then acos's argument)
            const F3 sp3 = sphere_pick_v8(rg);
            const F3 dir = normalized(add((f >> 31) ? neg(N) : N, sp3));  // scatterDiffuse about N or -N
            const uint32_t dst = j == 0 ? a.x : a.y;
            if (dst >= bound) continue;
            W.dx[dst] = dir.x;
            W.dy[dst] = dir.y;
            W.dz[dst] = dir.z;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) *W.fixctr = 0u;  // the next level's records
}

__global__ __launch_bounds__(256) void k_resolve_paths(RenderArgs A, WArgs W) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q >= W.npaths || W.lvl[LVL_FLAG]) return;
    const F3 v = resolve_chain(A, W, q, 0);
    W.root[3 * q] = v.x;
    W.root[3 * q + 1] = v.y;
    W.root[3 * q + 2] = v.z;
}

// The colours of a batch of the caller's rays (k_gen_rays): path q's resolved colour to out[3 * (ray * spp + sample)],
// as it is -- no accumulation, no 1 / passes, no setColor.  Chain schedule: resolved here, as k_resolve does for one
// sample; tree and hybrid chain: from root (k_reduce / k_resolve_paths).  A poisoned batch writes nothing: the
// host redoes it, as it redoes a frame.
__global__ __launch_bounds__(256) void k_store_colors(RenderArgs A, WArgs W, RayFeed F) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q >= W.npaths || W.lvl[LVL_FLAG]) return;
    const uint32_t nb = W.npaths / W.npix;
    const F3 v = (W.chain && !W.hybrid) ? resolve_path(A, W, q) : f3(W.root[3 * q], W.root[3 * q + 1], W.root[3 * q + 2]);
    float *dst = F.out + 3 * ((size_t)(W.p0 + q / nb) * F.spp + W.s0 + q % nb);
    dst[0] = v.x;
    dst[1] = v.y;
    dst[2] = v.z;
}

// k_gen's ray computation with the ray as the output (Camera.getRayForPixel as a batch): pixel p = py * W + px of
// A's W x H, sample index `sample`; the jitter of the sampling renderers (renderers.js:95-96) and camera_ray's DOF
// draws come from the pre-root frame of key (seed, pixel, sample), as in k_gen
__global__ __launch_bounds__(256) void k_camera_rays(DScene S, RenderArgs A, uint32_t sample, float *out) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= (uint32_t)A.W * (uint32_t)A.H) return;
    const int py = (int)(p / (uint32_t)A.W), px = (int)(p % (uint32_t)A.W);
    Rng pre{mix32(mix32(A.seed, p), sample), 0u, 0u};
    double x = 2 * ((double)px / A.W) - 1, y = -2 * ((double)py / A.H) + 1;  // renderers.js:22-25
    if (A.kind != JSRT_RENDERER_SIMPLE) {
        const double jx = x + (2.0 / A.W) * (pre.next() - 0.5);
        const double jy = y + (2.0 / A.H) * (pre.next() - 0.5);
        x = jx;
        y = jy;
    }
    F3 o, d;
    camera_ray(S.cam, x, y, pre, o, d);
    float *r = out + 6 * (size_t)p;
    r[0] = o.x; r[1] = o.y; r[2] = o.z;
    r[3] = d.x; r[4] = d.y; r[5] = d.z;
}

__global__ __launch_bounds__(256) void k_final(RenderArgs A, int32_t passes) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= (uint32_t)A.ncols * A.H) return;
    const F3 acc = f3(A.accum[4 * p], A.accum[4 * p + 1], A.accum[4 * p + 2]);
    const F3 out = (A.kind == JSRT_RENDERER_INCREMENTAL) ? scale(acc, 1.0 / passes) : acc;  // times(1/(iter+1))
    A.rgba[p] = set_color_rgba(out);
    if (A.colors) {
        A.colors[4 * p] = out.x;
        A.colors[4 * p + 1] = out.y;
        A.colors[4 * p + 2] = out.z;
        A.colors[4 * p + 3] = 1.0f;
    }
}

// ---------------------------------------------------------------------------------------------
// host orchestration
void EventPairs::begin(hipStream_t s) {
    if (used == b.size()) {
        hipEvent_t x, y;
        (void)hipEventCreate(&x);
        (void)hipEventCreate(&y);
        b.push_back(x);
        e.push_back(y);
    }
    (void)hipEventRecord(b[used], s);
}
void EventPairs::end(hipStream_t s) { (void)hipEventRecord(e[used++], s); }
double EventPairs::total_ms(uint32_t *lost) const {
    double ms = 0;
    for (size_t k = 0; k < used; ++k) {
        float x = 0;
        if (hipEventElapsedTime(&x, b[k], e[k]) == hipSuccess) ms += x;
        else if (lost) ++*lost;
    }
    return ms;
}
EventPairs::~EventPairs() {
    for (auto x : b) (void)hipEventDestroy(x);
    for (auto x : e) (void)hipEventDestroy(x);
}

// The run-time knobs (FrameKnobs, render_plan.h) from the environment: read once per frame, the only getenv of this file.
static FrameKnobs frame_knobs() {
    auto is1 = [](const char *n) { const char *v = getenv(n); return v ? (v[0] == '1' ? 1 : 0) : -1; };  // -1 unset
    auto not0 = [](const char *n) { const char *v = getenv(n); return !(v && v[0] == '0'); };
    FrameKnobs K;
    const char *v;
    K.force_exact_pick = is1("JSRT_FORCE_EXACT_PICK") == 1;
    if ((v = getenv("JSRT_FIX_CAP"))) K.fix_cap = std::max(0, atoi(v));
    if ((v = getenv("JSRT_HYBRID"))) K.hybrid = v[0] == '0' ? 0 : 1;
    K.pixel_major = is1("JSRT_PIXEL_MAJOR");
    if ((v = getenv("JSRT_BATCH_SPP"))) K.batch_spp = (uint32_t)std::max(1, atoi(v));
    if ((v = getenv("JSRT_TILE_PATCHES"))) K.tile_patches = std::max(0, atoi(v));
    K.persist = not0("JSRT_PERSIST");
    K.split_frame = not0("JSRT_SPLIT_FRAME");
    if ((v = getenv("JSRT_SPLIT_MIN"))) K.split_min = std::max(1, std::min(40, atoi(v)));
    if ((v = getenv("JSRT_SPLIT_PIXELS"))) K.split_pixels = v[0] == '1';
    if ((v = getenv("JSRT_POOL_FACTOR"))) K.pool_factor = (size_t)std::max(1, atoi(v));
    if ((v = getenv("JSRT_BOUND_MARGIN"))) {
        K.bound_margin = atof(v);
        K.bound_slack = 0;
    }
    K.dual = is1("JSRT_DUAL");
    K.split = is1("JSRT_SPLIT");
    K.shadow_serial = is1("JSRT_SHADOW_SERIAL") == 1;
    K.shadow_node = is1("JSRT_SHADOW_NODE") != 0;
    K.bucket = not0("JSRT_BUCKET");
    K.child_sort = is1("JSRT_CHILD_SORT");
    K.bucket_grid = is1("JSRT_BUCKET_GRID");
    return K;
}

hipError_t Wavefront::reserve(const PoolDims &d, const FrameKnobs &K) {
    const size_t fixcap = fix_capacity(learned.fix_all, d.rays, K);
    const size_t bytes = pool_bytes(d, fixcap);
    if (!mem || bytes > cap_bytes) {  // (else: carve the cached allocation again)
        if (mem) (void)hipFree(mem);
        mem = nullptr;
        cap_bytes = 0;
        hipError_t e = hipMalloc(&mem, bytes);
        if (e != hipSuccess) return e;
        cap_bytes = bytes;
    }
    carve_pool(args, d, fixcap, static_cast<uint8_t *>(mem));
    args.force_fix = K.force_exact_pick ? 1 : 0;
    return hipSuccess;
}

void Wavefront::release() {
    if (mem) (void)hipFree(mem);
    mem = nullptr;
    cap_bytes = 0;
    if (twin) twin->release();
}

Wavefront::~Wavefront() {
    release();
    delete twin;
    if (side) (void)hipStreamDestroy(side);
    if (aux) (void)hipStreamDestroy(aux);
    if (ev_shade) (void)hipEventDestroy(ev_shade);
    if (ev_shadow) (void)hipEventDestroy(ev_shadow);
}

size_t wavefront_bytes_per_path(const DScene &S, int ns, int max_depth) {
    return pool_bytes_per_path(S, ns, max_depth, schedule_of(S, frame_knobs()));
}

// Grid of a persistent kernel: as many 256-thread blocks as the device keeps resident (occupancy x
// CUs), never more than the work needs.  Cached per kernel and device behind a mutex: renders run
// concurrently on several host threads (Node async work, worker threads, one scene per thread).
unsigned persistent_grid(const void *kernel, size_t work) {
    static std::mutex mu;
    static std::vector<std::pair<std::pair<const void *, int>, unsigned>> cache;
    int dev = 0;
    (void)hipGetDevice(&dev);
    unsigned resident = 0;
    {
        std::lock_guard<std::mutex> lk(mu);
        for (auto &c : cache)
            if (c.first.first == kernel && c.first.second == dev) resident = c.second;
    }
    if (!resident) {
        int per_cu = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0) != hipSuccess || per_cu < 1) per_cu = 1;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
        resident = (unsigned)(per_cu * cus);
        std::lock_guard<std::mutex> lk(mu);
        cache.push_back({{kernel, dev}, resident});
    }
    return std::max(1u, std::min(resident, grid_ub(work)));
}

// instantiated in render_pf.hip, one translation unit per profile
#define JSRT_PF_EXTERN(PFV)                                                                                            \
    extern template void run_batch<PFV, true>(const DScene &, const RenderArgs &, const WArgs &, hipStream_t,          \
                                              KernelTimes *, const std::vector<size_t> &, const BatchSync *);          \
    extern template void run_batch<PFV, false>(const DScene &, const RenderArgs &, const WArgs &, hipStream_t,         \
                                               KernelTimes *, const std::vector<size_t> &, const BatchSync *);         \
    extern template void cast_rays_pf<PFV>(const DScene &, const float *, uint32_t, double, double, int, double *,     \
                                           int32_t *, hipStream_t);                                                    \
    extern template bool cast_path_pf<PFV>(const DScene &, int, const float *, uint32_t, double, double, int,          \
                                           uint32_t *, double *, int32_t *, hipStream_t);                              \
    extern template void material_data_pf<PFV>(const DScene &, const float *, uint32_t, double *, int32_t *, float *,  \
                                               float *, float *, float *, float *, hipStream_t);                       \
    extern template void material_uv_pf<PFV>(const DScene &, const float *, uint32_t, float *, int32_t *, hipStream_t);
JSRT_PF_EXTERN(PF_ANALYTIC)
JSRT_PF_EXTERN(PF_MESH)
JSRT_PF_EXTERN(PF_SDF)
JSRT_PF_EXTERN(PF_ALL)
#undef JSRT_PF_EXTERN

// f(std::integral_constant<int, PF>) for the scene's kernel profile: the one switch over the instantiations above
template <class F>
static void with_profile(int profile, F &&f) {
    switch (profile) {
    case PF_ANALYTIC: f(std::integral_constant<int, PF_ANALYTIC>{}); break;
    case PF_MESH: f(std::integral_constant<int, PF_MESH>{}); break;
    case PF_SDF: f(std::integral_constant<int, PF_SDF>{}); break;
    default: f(std::integral_constant<int, PF_ALL>{}); break;
    }
}

hipError_t material_data_rays(const DScene &S, const float *d_rays, uint32_t n, double *d_t, int32_t *d_prim,
                              float *d_nrm, float *d_pos, float *d_uv, float *d_bary, float *d_bc, hipStream_t st) {
    if (n == 0) return hipSuccess;
    with_profile(S.profile, [&](auto pf) {
        material_data_pf<decltype(pf)::value>(S, d_rays, n, d_t, d_prim, d_nrm, d_pos, d_uv, d_bary, d_bc, st);
    });
    return hipGetLastError();
}

hipError_t material_uv_rays(const DScene &S, const float *d_rays, uint32_t n, float *d_uv, int32_t *d_has, hipStream_t st) {
    if (n == 0) return hipSuccess;
    with_profile(S.profile, [&](auto pf) { material_uv_pf<decltype(pf)::value>(S, d_rays, n, d_uv, d_has, st); });
    return hipGetLastError();
}

// SDF.distance of SDF geometry g's root (sdf.js:53-74) at points (f32 x 4, w = 1): the same program VM
// the render's march runs (jsrt_sdf_distance)
__global__ __launch_bounds__(256) void k_sdf_distance(DScene S, int g, const float *pts, uint32_t n, double *out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float *p = pts + 4 * (size_t)i;
    out[i] = sdf_node_dist(S, S.sdfg[g].root, f3(p[0], p[1], p[2]));
}

hipError_t sdf_distance_points(const DScene &S, int g, const float *d_pts, uint32_t n, double *d_out, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sdf_distance, dim3(grid_ub(n)), dim3(256), 0, st, S, g, d_pts, n, d_out);
    return hipGetLastError();
}

// MaterialColor.color({UV: uv}) of one MCOL record (solid, scaled, checkerboard or texture chain), one lane per
// UV pair: mc_eval with the sampler, as k_shade's TEX instantiation runs it (jsrt_material_color)
__global__ __launch_bounds__(256) void k_material_color(DScene S, int mc, const float *uv, uint32_t n, float *rgb) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const F3 c = mc_eval<true>(S, mc, uv[2 * (size_t)i], uv[2 * (size_t)i + 1]);
    float *o = rgb + 3 * (size_t)i;
    o[0] = c.x;
    o[1] = c.y;
    o[2] = c.z;
}

hipError_t material_color_uvs(const DScene &S, int mc, const float *d_uv, uint32_t n, float *d_rgb, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_material_color, dim3(grid_ub(n)), dim3(256), 0, st, S, mc, d_uv, n, d_rgb);
    return hipGetLastError();
}

hipError_t cast_rays(const DScene &S, const float *d_rays, uint32_t n, double min_dist, double max_dist, bool transparent,
                     double *d_t, int32_t *d_prim, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const int tr = transparent ? 1 : 0;
    with_profile(S.profile, [&](auto pf) { cast_rays_pf<decltype(pf)::value>(S, d_rays, n, min_dist, max_dist, tr, d_t, d_prim, st); });
    return hipGetLastError();
}

hipError_t cast_rays_path(const DScene &S, int path, const float *d_rays, uint32_t n, double min_dist, double max_dist,
                          bool transparent, uint32_t *d_ctr, double *d_t, int32_t *d_prim, hipStream_t st, bool *have) {
    *have = true;
    if (n == 0) return hipSuccess;
    const int tr = transparent ? 1 : 0;
    // the persistent march serves SDF scenes whose roots are all Primitives (plan_batches' `persist`), the
    // node-per-lane shadow cast flat scenes (every root a Primitive, no SDF: cast_path_pf)
    if ((path == CAST_PATH_PERSISTENT || path == CAST_PATH_PERSISTENT_ANY || path == CAST_PATH_ANY_NODE) && !S.all_roots_prims) {
        *have = false;
        return hipSuccess;
    }
    with_profile(S.profile, [&](auto pf) {
        *have = cast_path_pf<decltype(pf)::value>(S, path, d_rays, n, min_dist, max_dist, tr, d_ctr, d_t, d_prim, st);
    });
    return hipGetLastError();
}

namespace {
// What a frame holds on the host beside its pools: the pinned read-back of the level counts (tree / hybrid
// schedule) and the frame flags of both pools, and the four events that order the two batch streams.  Freed on
// every exit of trace_frame.
struct FrameHost {
    uint32_t *h_lvl = nullptr;
    hipEvent_t ev_start = nullptr, ev_end = nullptr, ev_acc[2] = {nullptr, nullptr};
    ~FrameHost() {
        if (h_lvl) (void)hipHostFree(h_lvl);
        for (hipEvent_t x : {ev_start, ev_end, ev_acc[0], ev_acc[1]})
            if (x) (void)hipEventDestroy(x);
    }
};
}  // namespace

// The batches of a frame of npix_total pixels (run_frame below), attempt after attempt until none is poisoned.  The
// arithmetic -- plan, schedule, pool shape, launch bounds, settings, what a redo changes -- is render_plan.h's; here
// are the streams, the events, the twin pool, the memsets, the batch loop and the read-back of the flags.
// aborted: the callback ended the frame, which is then left as the last preview had it.
static hipError_t trace_frame(const DScene &S, const RenderArgs &A, int ns, Wavefront &wf, hipStream_t st, KernelTimes *kt,
                              size_t max_paths, const std::function<bool(int, double, bool)> &progress,
                              const std::function<bool()> &due, const RayFeed *feed, uint32_t npix_total, bool &aborted) {
    const FrameKnobs K = frame_knobs();  // per frame: a process may change its environment between renders
    const BatchPlan plan = plan_batches(S, A, ns, max_paths, K);
    RenderArgs At = A;
    At.tile_p = plan.tile_p;
    // Chain schedule when no node can have two children: depth x paths node records, nothing can
    // overflow, batches are enqueued back to back.  Tree schedule otherwise: a ray pool for all
    // levels of a batch (one level may hold half of it), compacted level by level.  Its launches
    // are sized by level counts learned from the scene's first batch (one read-back per scene and
    // batch shape) with a margin; a batch that outgrows its pool (LVL_FLAG) or a launch bound
    // (LVL_UNDER) poisons the frame, which is redone with a larger pool / conservative bounds.
    // The frame flags are read once, after the last batch.
    // Hybrid chain (branching materials, the default): the chain layout -- ray slot = path, node [L * cap +
    // slot], no parent / path planes, one bottom-up resolve -- plus a side chain per second child (a slot
    // appended after the paths, cap = paths + paths x pool_factor / 4).  Its level counts (the side chains
    // started so far) live on the device; launch bounds, overflow and redo work as for the tree.
    const int sched = schedule_of(S, K);
    const bool hybrid = sched == SCHED_HYBRID, chain = sched != SCHED_TREE, learned = sched != SCHED_CHAIN;
    const int depth = std::max(1, A.max_depth);
    const size_t paths = (size_t)plan.npix * plan.nsb;
    LearnedPool &lp = wf.learned;
    if (learned && (lp.pool_paths != paths || lp.pool_mode != sched)) {  // learned pool / bounds: per batch shape
        lp.pool_factor = initial_pool_factor(sched, paths, K);
        lp.frac.clear();
        lp.pool_paths = paths;
        lp.pool_mode = sched;
    }
    hipError_t e = hipSuccess;
    FrameHost H;
    if ((e = hipHostMalloc((void **)&H.h_lvl, 128 * sizeof(uint32_t), 0)) != hipSuccess) return e;
    // Two batch pools on two streams: consecutive batches alternate between them, so one batch's levels
    // (latency-bound casts, VALU-bound shadow samples, their launch tails) overlap the other's.  Only the
    // accumulation into A.accum is ordered across them -- each batch's k_accum / k_resolve waits for the
    // previous batch's (renderers.js:93-97: samples in order) -- so the image is unchanged bit for bit.
    // (A/B on MI355X, profiles/r03_s18_ab.txt: cornell +12.5 %, the dragon +2.6 %, bunny +0.6 %; two
    // persistent SDF marches side by side lose 1 %, so SDF scenes with persistent casts run on one
    // stream.)  The twin pool is allocated only if it fits; otherwise the frame runs on one pool.
    const uint32_t rows = batch_rows(plan, (uint32_t)A.spp), cols = batch_cols(plan, npix_total);  // render_plan.h
    const uint64_t nbatches = (uint64_t)rows * cols;
    // A render that asks for its launches' own times (JSRT_EVENTS_ONE_STREAM) runs on one stream: a
    // launch's event interval is only its own time when no other batch's kernels share the CUs.
    const bool timed_launches = kt && kt->one_stream;
    // two streams need two batches of comparable size (render_plan.h two_full)
    bool dual = !timed_launches && nbatches > 1 &&
                (K.dual >= 0 ? K.dual == 1 : (!plan.persist && two_full(plan, npix_total, (uint32_t)A.spp)));
    if (dual) {
        if (!wf.twin) wf.twin = new Wavefront();
        if (!wf.side) e = hipStreamCreateWithFlags(&wf.side, hipStreamNonBlocking);
        for (hipEvent_t *x : {&H.ev_start, &H.ev_end, &H.ev_acc[0], &H.ev_acc[1]})
            if (e == hipSuccess) e = hipEventCreateWithFlags(x, hipEventDisableTiming);
        if (e != hipSuccess) return e;
    }
    hipStream_t st2 = dual ? wf.side : st;
    // A frame with persistent SDF casts (one stream) runs k_shadow on a stream of its own (BatchSync::aux):
    // level L's shadow samples overlap level L + 1's march.  SDF_Menger +6.5 %; elsewhere it loses
    // (bunny on one stream -5 %; beside two batch streams cornell +-0, dragon -1.3 %; profiles/
    // r03_s18_ab.txt s22, s26).  JSRT_SPLIT=0/1 forces it.
    const bool split = !timed_launches && ns > 0 && (K.split >= 0 ? K.split == 1 : (plan.persist && !dual));
    auto aux_of = [&](Wavefront &w) -> hipError_t {
        hipError_t r = hipSuccess;
        if (!w.aux) r = hipStreamCreateWithFlags(&w.aux, hipStreamNonBlocking);
        if (r == hipSuccess && !w.ev_shade) r = hipEventCreateWithFlags(&w.ev_shade, hipEventDisableTiming);
        if (r == hipSuccess && !w.ev_shadow) r = hipEventCreateWithFlags(&w.ev_shadow, hipEventDisableTiming);
        return r;
    };
    if (split && (e = aux_of(wf)) == hipSuccess && dual) e = aux_of(*wf.twin);
    if (e != hipSuccess) return e;
    bool conservative = false;
    double reported = 0;  // completion already reported: a redone frame reports only beyond it
    for (int attempt = 0; e == hipSuccess; ++attempt) {
        if (kt) kt->attempts = (uint32_t)attempt + 1;
        const PoolShape shape = pool_shape(sched, paths, depth, lp.pool_factor, ns, plan.persist, K);
        if (!shape.fits) { e = hipErrorOutOfMemory; break; }  // u32 node index
        e = wf.reserve(shape.dims, K);
        if (e == hipSuccess && dual) {
            const hipError_t e2 = wf.twin->reserve(shape.dims, K);
            if (e2 == hipErrorOutOfMemory) {  // no room for a second pool: one pool, one stream
                (void)hipGetLastError();
                wf.twin->release();
                dual = false;
                st2 = st;
            } else {
                e = e2;
            }
        }
        if (e != hipSuccess) break;
        WArgs W = wf.args;
        batch_settings(W, S, K, plan, shape, ns, sched);
        WArgs W2 = W;  // the twin pool: the same settings over its own buffers
        if (dual) {
            W2 = wf.twin->args;
            batch_settings(W2, S, K, plan, shape, ns, sched);
        }
        if (!feed && (e = hipMemsetAsync(A.accum, 0, (size_t)A.ncols * A.H * 4 * sizeof(float), st)) != hipSuccess) break;
        if ((e = hipMemsetAsync(W.lvl + LVL_UNDER, 0, 2 * sizeof(uint32_t), st)) != hipSuccess) break;  // frame flags
        if ((e = hipMemsetAsync(W.fixctr, 0, sizeof(uint32_t), st)) != hipSuccess) break;
        if (dual && (e = hipMemsetAsync(W2.fixctr, 0, sizeof(uint32_t), st)) != hipSuccess) break;
        if (dual) {  // the side stream starts after everything enqueued on st so far
            if ((e = hipEventRecord(H.ev_start, st)) != hipSuccess || (e = hipStreamWaitEvent(st2, H.ev_start, 0)) != hipSuccess) break;
            if ((e = hipMemsetAsync(W2.lvl + LVL_UNDER, 0, 2 * sizeof(uint32_t), st2)) != hipSuccess) break;
        }
        // the frame flags (and, for progress, level counts) of both pools, read back after both streams idle
        auto read_flags = [&]() -> hipError_t {
            hipError_t r;
            if (dual && ((r = hipEventRecord(H.ev_end, st2)) != hipSuccess || (r = hipStreamWaitEvent(st, H.ev_end, 0)) != hipSuccess))
                return r;
            if ((r = hipMemcpyAsync(H.h_lvl, W.lvl, 64 * sizeof(uint32_t), hipMemcpyDeviceToHost, st)) != hipSuccess) return r;
            if (dual && (r = hipMemcpyAsync(H.h_lvl + 64, W2.lvl, 64 * sizeof(uint32_t), hipMemcpyDeviceToHost, st)) != hipSuccess)
                return r;
            return hipStreamSynchronize(st);
        };
        auto flagged = [&](int k) { return H.h_lvl[k] != 0 || (dual && H.h_lvl[64 + k] != 0); };
        uint64_t bi = 0;  // batch index: even batches on (W, st), odd ones on (W2, st2)
        const uint64_t total = (uint64_t)npix_total * A.spp;
        uint64_t done = 0;
        // stop: the callback aborted the frame.  redo_now: a progress check found a batch poisoned -- the frame is
        // redone at once instead of after its last batch, so that every pass is reported exactly once and from a
        // clean frame (a multi-rank caller keeps its collectives in step on the passes, tiles.render_progressive)
        bool stop = false, redo_now = false;
        // A due callback: wait for the batches so far and report `pass` from a clean frame.  false ends the batch
        // loop (an error in e, a poisoned batch, or the callback's abort).
        auto report = [&](int pass) {
            if ((e = read_flags()) != hipSuccess) return false;
            if (flagged(LVL_FLAG) || flagged(LVL_UNDER)) {
                redo_now = true;
                return false;
            }
            const double c = (double)done / (double)total;
            if (c > reported) {
                reported = c;
                stop = !progress(pass, c, true);
            }
            return !stop;
        };
        for (uint32_t row = 0; row < rows && e == hipSuccess && !stop && !redo_now; ++row) {
            const BatchSpan r0 = batch_span(plan, npix_total, (uint32_t)A.spp, row, 0);
            const uint32_t s0 = r0.s0, nb = r0.nb;  // the row's samples
            for (uint32_t col = 0; col < cols; ++col, ++bi) {
                const BatchSpan span = batch_span(plan, npix_total, (uint32_t)A.spp, row, col);
                const bool odd = dual && (bi & 1);
                WArgs &Wb = odd ? W2 : W;
                const hipStream_t sb = odd ? st2 : st;
                Wb.p0 = span.p0;
                Wb.npix = span.npix;
                Wb.s0 = span.s0;
                Wb.npaths = span.npix * span.nb;
                Wb.cap = hybrid ? (uint32_t)shape.cap : Wb.npaths;
                const std::vector<size_t> bound =
                    learned ? level_bounds(sched, Wb.npaths, shape, A.max_depth, S.max_children, lp.frac, conservative, K)
                            : std::vector<size_t>();
                BatchSync sync;
                sync.feed = feed;
                if (dual) {
                    sync.wait = bi > 0 ? H.ev_acc[(bi - 1) & 1] : nullptr;
                    sync.done = H.ev_acc[bi & 1];
                }
                if (split) {
                    Wavefront &pw = odd ? *wf.twin : wf;
                    sync.aux = pw.aux;
                    sync.shade_done = pw.ev_shade;
                    sync.shadow_done = pw.ev_shadow;
                }
                with_profile(S.profile, [&](auto pf) {
                    if (chain) run_batch<decltype(pf)::value, true>(S, At, Wb, sb, kt, bound, &sync);
                    else run_batch<decltype(pf)::value, false>(S, At, Wb, sb, kt, bound, &sync);
                });
                if ((e = hipGetLastError()) != hipSuccess) break;
                done += (uint64_t)Wb.npix * nb;
                if (kt) ++kt->batches;
                // Simple / RandomMultisampling report {pass: 0, completion: pixels done / total} from inside
                // their pixel loop (renderers.js:28-37): here after a batch, when a callback is due (the
                // host's timelimit clock is checked first: no sync otherwise)
                if (progress && A.kind != JSRT_RENDERER_INCREMENTAL && (!due || due()) && !report(0)) break;
                if (learned && (lp.frac.empty() || conservative)) {
                    // learn the level counts: from the scene's first batch, or -- when that batch was
                    // not representative and a frame had to be redone -- as the maximum over every
                    // batch of the conservative redo, so later frames of this shape are not redone
                    if ((e = hipMemcpyAsync(H.h_lvl, Wb.lvl, 64 * sizeof(uint32_t), hipMemcpyDeviceToHost, sb)) != hipSuccess) break;
                    if ((e = hipStreamSynchronize(sb)) != hipSuccess) break;
                    learn_fractions(lp.frac, H.h_lvl, A.max_depth, hybrid, Wb.npaths);
                }
            }
            // Incremental: wait for the pass
            if (e == hipSuccess && progress && A.kind == JSRT_RENDERER_INCREMENTAL && (!due || due()) && !report((int)(s0 + nb - 1)))
                break;
        }
        if (e != hipSuccess) break;
        if (stop) {  // an aborted frame is not redone (read_flags joins the side stream into st and waits for it)
            e = read_flags();
            aborted = true;
            break;
        }
        // The frame flags of both pools, every schedule.  read_flags also joins the side stream into st, so the
        // caller's stream orders after every batch of the frame (k_final, and the caller's own work after
        // jsrt_render_device returns).  A frame that ended with a batch poisoned is redone, never returned: in
        // the round-4 draft of the hybrid chain this loop broke out for every chain-layout schedule before
        // reading the flags, so a hybrid frame whose side chains outgrew their slots came back with its
        // poisoned batches' pixels missing (tests/test_gpu_redo_streams.py).
        if ((e = read_flags()) != hipSuccess) break;
        const bool flag = flagged(LVL_FLAG), under = flagged(LVL_UNDER);
        if (!flag && !under) break;
        if (redo_step(lp, wf.twin ? &wf.twin->learned.fix_all : nullptr, sched, paths, flag, under, conservative) ==
            Redo::OUT_OF_MEMORY) {
            e = hipErrorOutOfMemory;
            break;
        }
        if (kt) kt->reset();
    }
    if (e != hipSuccess && dual) {  // nothing of this frame may still run on the side stream
        (void)hipStreamSynchronize(st2);
        (void)hipStreamSynchronize(st);
    }
    return e;
}

// A frame's batches: the camera's paths of the owned pixels into A.accum (render_frame), or -- feed -- World.color of
// the caller's rays into feed->out (color_frame), where a "pixel" of the plan is a ray and nothing of the pixel order
// (pixel_of, tiles, column ownership) is involved.  One plan, level loop, pools, streams and redo logic for both.
static hipError_t run_frame(const DScene &S, const RenderArgs &A, int ns, Wavefront &wf, hipStream_t st, KernelTimes *kt,
                            size_t max_paths, const std::function<bool(int, double, bool)> &progress,
                            const std::function<bool()> &due, const RayFeed *feed) {
    if (!feed && !A.accum) return hipErrorInvalidValue;
    const uint32_t npix_total = feed ? feed->n : (uint32_t)A.patches * 64u;
    if (npix_total == 0) {  // a rank that owns no column (a multi-GPU frame narrower than its column blocks):
        // nothing to trace, but an Incremental frame's passes are still reported, so that the rank's callbacks
        // keep step with its peers' (tiles.render_progressive runs one collective per reported pass)
        if (progress && A.kind == JSRT_RENDERER_INCREMENTAL) {
            const uint32_t step = A.samples_per_batch > 0 ? (uint32_t)A.samples_per_batch : (uint32_t)A.spp;
            for (uint32_t s_end = step; s_end < (uint32_t)A.spp; s_end += step)
                if ((!due || due()) && !progress((int)s_end - 1, (double)s_end / A.spp, true)) break;
        }
        return hipSuccess;
    }
    bool aborted = false;
    const hipError_t e = trace_frame(S, A, ns, wf, st, kt, max_paths, progress, due, feed, npix_total, aborted);
    if (e != hipSuccess) return e;
    // an aborted frame leaves the caller's tile as the last preview left it (no k_final over a partial
    // accumulator), with the device idle (read_flags waited): jsrt.h's -4 contract
    if (aborted) return hipSuccess;
    if (!A.rgba) return hipSuccess;  // the caller takes the accumulator itself (jsrt_render_device_accum)
    const bool ev = kt && kt->on(KT_FINAL);
    if (ev) kt->ev[KT_FINAL].begin(st);
    hipLaunchKernelGGL(k_final, dim3(grid((size_t)A.ncols * A.H)), dim3(256), 0, st, A, (int32_t)A.spp);
    if (ev) kt->ev[KT_FINAL].end(st);
    return hipGetLastError();
}

hipError_t render_frame(const DScene &S, const RenderArgs &A, int ns, Wavefront &wf, hipStream_t st, KernelTimes *kt,
                        size_t max_paths, const std::function<bool(int, double, bool)> &progress,
                        const std::function<bool()> &due) {
    return run_frame(S, A, ns, wf, st, kt, max_paths, progress, due, nullptr);
}

hipError_t color_frame(const DScene &S, const RenderArgs &A, const RayFeed &F, int ns, Wavefront &wf, hipStream_t st,
                       KernelTimes *kt, size_t max_paths) {
    if (F.n == 0 || F.spp == 0) return hipSuccess;
    if ((!F.rays && !F.cams) || !F.out || A.max_depth < 0 || A.max_depth > MAX_TREE_DEPTH) return hipErrorInvalidValue;
    if (A.max_depth == 0)  // World.color(ray, 0) = black (world.js:32): nothing is traced
        return hipMemsetAsync(F.out, 0, (size_t)F.n * F.spp * 3 * sizeof(float), st);
    RenderArgs Ar{};  // what the plan and the kernels after the first read of a frame: the batch grid, depth and seed
    Ar.max_depth = A.max_depth;
    Ar.seed = A.seed;
    Ar.spp = (int32_t)F.spp;
    Ar.kind = JSRT_RENDERER_RANDOM;  // (no pass structure: nothing is reported)
    if (F.cams) {  // a view batch: the frame size and the renderer kind (its jitter), as k_gen reads them
        Ar.W = A.W;
        Ar.H = A.H;
        Ar.kind = A.kind;
    }
    Ar.patches = (int32_t)(((uint64_t)F.n + 63) / 64);  // the plan's pixel count, in whole 64s
    return run_frame(S, Ar, ns, wf, st, kt, max_paths, nullptr, nullptr, &F);
}

hipError_t camera_rays(const DScene &S, const RenderArgs &A, uint32_t sample, float *d_rays, hipStream_t st) {
    const size_t n = (size_t)A.W * A.H;
    if (n == 0) return hipSuccess;
    if (!d_rays || n > (size_t)UINT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_camera_rays, dim3(grid(n)), dim3(256), 0, st, S, A, sample, d_rays);
    return hipGetLastError();
}

hipError_t finish_accum(const float *accum, size_t n, int kind, int passes, uint32_t *rgba, float *colors, hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (!accum || !rgba || passes < 1 || n > (size_t)INT32_MAX) return hipErrorInvalidValue;
    RenderArgs A{};
    A.kind = kind;
    A.ncols = (int32_t)n;
    A.H = 1;
    A.accum = const_cast<float *>(accum);
    A.rgba = rgba;
    A.colors = colors;
    hipLaunchKernelGGL(k_final, dim3(grid(n)), dim3(256), 0, st, A, (int32_t)passes);
    return hipGetLastError();
}

hipError_t render_preview(const RenderArgs &A, int passes, hipStream_t st) {
    if (!A.accum || !A.rgba || passes < 1) return hipErrorInvalidValue;
    if ((size_t)A.ncols * A.H == 0) return hipSuccess;
    hipLaunchKernelGGL(k_final, dim3(grid((size_t)A.ncols * A.H)), dim3(256), 0, st, A, (int32_t)passes);
    return hipGetLastError();
}


}  // namespace jsrt
