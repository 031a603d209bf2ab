// Host build of the frame driver's arithmetic (jsraytracer_amd/csrc/render_plan.h: schedule_of, initial_pool_factor,
// pool_shape, level_bounds, batch_settings, learn_fractions, redo_step, fix_capacity, the pool layout and
// pool_bytes_per_path) for tests/test_frame_policy.py.  Every entry takes and returns arrays of long long.
#include <string.h>

#include "../../jsraytracer_amd/csrc/render_plan.h"

using namespace jsrt;
typedef long long ll;

static FrameKnobs knobs_of(const ll *k) {  // {fix_cap (-1 unset), force_exact_pick, shadow_serial, pool_factor}
    FrameKnobs K;
    K.fix_cap = (int)k[0];
    K.force_exact_pick = k[1] != 0;
    K.shadow_serial = k[2] != 0;
    K.pool_factor = (size_t)k[3];
    return K;
}

extern "C" ll schedule(ll max_children, ll profile, ll hybrid_knob) {
    DScene S{};
    S.max_children = (int32_t)max_children;
    S.profile = (int32_t)profile;
    FrameKnobs K;
    K.hybrid = (int)hybrid_knob;
    return schedule_of(S, K);
}

extern "C" ll init_factor(ll sched, ll paths, const ll *knobs) {
    return (ll)initial_pool_factor((int)sched, (size_t)paths, knobs_of(knobs));
}

// out: {cap, pool, level_cap, group, hands, shadow, fits, dims: rays, nodes, hands, paths, mode, shadow}
extern "C" void shape(ll sched, ll paths, ll depth, ll factor, ll ns, ll persist, const ll *knobs, ll *out) {
    const PoolShape P = pool_shape((int)sched, (size_t)paths, (int)depth, (size_t)factor, (int)ns, persist != 0, knobs_of(knobs));
    const ll v[13] = {(ll)P.cap, (ll)P.pool, (ll)P.level_cap, P.group, (ll)P.hands, (ll)P.shadow, P.fits,
                      (ll)P.dims.rays, (ll)P.dims.nodes, (ll)P.dims.hands, (ll)P.dims.paths, P.dims.mode, (ll)P.dims.shadow};
    memcpy(out, v, sizeof v);
}

// The layout of PoolDims d = {rays, nodes, hands, paths, mode, shadow} with fix_all and the knobs.
// head: {pool_bytes, fix_capacity, WArgs::fixcap, nstride, hstride, sstride, words of WArgs that carve_pool left
// non-zero beside the buffers, the strides and fixcap}.  off / size, 31 each in the order of NAMES in the test: the
// buffer's offset from the base (-1: null) and the bytes it holds (elements x element size, as the layout's visitor
// is handed them; 0 when not visited).
extern "C" void layout(const ll *d, ll fix_all, const ll *knobs, ll *head, ll *off, ll *size) {
    const PoolDims D{(size_t)d[0], (size_t)d[1], (size_t)d[2], (size_t)d[3], (int)d[4], (size_t)d[5]};
    const FrameKnobs K = knobs_of(knobs);
    const size_t fixcap = fix_capacity(fix_all != 0, D.rays, K);
    WArgs w;
    memset(&w, 0xAB, sizeof w);  // carve_pool states every word
    uint8_t *const base = reinterpret_cast<uint8_t *>((uintptr_t)1 << 40);  // (not 0: a buffer at offset 0 is not null)
    carve_pool(w, D, fixcap, base);
    void *const fields[31] = {&w.ox, &w.oy, &w.oz, &w.dx, &w.dy, &w.dz, &w.addr, &w.key, &w.t, &w.prim, &w.ctx, &w.path,
                              &w.parent, &w.list0, &w.list1, &w.endl, &w.node, &w.child, &w.slot, &w.root, &w.hand,
                              &w.hnode, &w.lvl, &w.qctr, &w.fixrec, &w.fixctr, &w.sray, &w.scol, &w.bkt, &w.bbase, &w.brank};
    for (int i = 0; i < 31; ++i) {
        uint8_t *p;
        memcpy(&p, fields[i], sizeof p);
        off[i] = p ? (ll)(p - base) : -1;
        size[i] = 0;
    }
    WArgs seen = w;
    pool_fields(seen, D, fixcap, [&](auto *&p, size_t n) {
        const size_t at = (size_t)((char *)&p - (char *)&seen);
        for (int i = 0; i < 31; ++i)
            if ((size_t)((char *)fields[i] - (char *)&w) == at) size[i] = (ll)(n * sizeof(*p));
    });
    WArgs rest = w;
    for (int i = 0; i < 31; ++i) memset((char *)&rest + ((char *)fields[i] - (char *)&w), 0, sizeof(void *));
    rest.fixcap = 0;
    rest.nstride = rest.hstride = rest.sstride = 0;
    ll stray = 0;
    for (size_t i = 0; i < sizeof rest; ++i) stray += ((const unsigned char *)&rest)[i] != 0;
    head[0] = (ll)pool_bytes(D, fixcap);
    head[1] = (ll)fixcap;
    head[2] = w.fixcap;
    head[3] = (ll)w.nstride;
    head[4] = (ll)w.hstride;
    head[5] = (ll)w.sstride;
    head[6] = stray;
}

// level_bounds of a batch of np paths in a pool of `paths` paths at `factor`; margin_slack: {margin x 1e6, slack};
// out: max(1, max_depth) bounds; returns their number.
extern "C" ll bounds(ll sched, ll np, ll paths, ll max_depth, ll factor, ll max_children, const double *frac, ll nfrac,
                     ll conservative, double margin, ll slack, ll *out) {
    FrameKnobs K;
    K.bound_margin = margin;
    K.bound_slack = (size_t)slack;
    const PoolShape P = pool_shape((int)sched, (size_t)paths, (int)std::max<ll>(1, max_depth), (size_t)factor, 0, false, K);
    const std::vector<double> f(frac, frac + nfrac);
    const std::vector<size_t> b = level_bounds((int)sched, (uint32_t)np, P, (int)max_depth, (int)max_children, f, conservative != 0, K);
    for (size_t i = 0; i < b.size(); ++i) out[i] = (ll)b[i];
    return (ll)b.size();
}

// redo_step.  st (in / out): {pool_factor, fix_all, twin present, twin fix_all, frac entries, conservative};
// returns 0 redo, 1 out of memory.
extern "C" ll redo(ll *st, ll sched, ll paths, ll flag, ll under) {
    LearnedPool lp;
    lp.pool_factor = (size_t)st[0];
    lp.fix_all = st[1] != 0;
    bool twin_fix_all = st[3] != 0, conservative = st[5] != 0;
    lp.frac.assign((size_t)st[4], 0.5);
    const Redo r = redo_step(lp, st[2] ? &twin_fix_all : nullptr, (int)sched, (size_t)paths, flag != 0, under != 0, conservative);
    st[0] = (ll)lp.pool_factor;
    st[1] = lp.fix_all;
    st[3] = twin_fix_all;
    st[4] = (ll)lp.frac.size();
    st[5] = conservative;
    return r == Redo::OUT_OF_MEMORY ? 1 : 0;
}

// learn_fractions over frac (nfrac entries in, room for max_depth); returns the entries out
extern "C" ll learn(double *frac, ll nfrac, const unsigned *lvl, ll max_depth, ll hybrid, ll npaths) {
    std::vector<double> f(frac, frac + nfrac);
    learn_fractions(f, lvl, (int)max_depth, hybrid != 0, (uint32_t)npaths);
    for (size_t i = 0; i < f.size(); ++i) frac[i] = f[i];
    return (ll)f.size();
}

// batch_settings.  in: {profile, n_prims, grid_cells, sched, persist, pixel_major, ns, paths, depth, factor,
// knobs: shadow_node, bucket, child_sort, bucket_grid}.  out: {ns, group, shadow_node, chain, hybrid, cap, bucket,
// pool, level_cap, child_sort, bucket_grid, pixel_major, bytes of the WArgs changed beside these words}
extern "C" void settings(const ll *in, ll *out) {
    DScene S{};
    S.profile = (int32_t)in[0];
    S.n_prims = (int32_t)in[1];
    S.grid_cells = (int32_t)in[2];
    const int sched = (int)in[3], ns = (int)in[6];
    BatchPlan plan{};
    plan.persist = in[4] != 0;
    plan.pixel_major = in[5] != 0;
    FrameKnobs K;
    K.shadow_node = in[10] != 0;
    K.bucket = in[11] != 0;
    K.child_sort = (int)in[12];
    K.bucket_grid = (int)in[13];
    const PoolShape P = pool_shape(sched, (size_t)in[7], (int)in[8], (size_t)in[9], ns, plan.persist, K);
    WArgs before;
    memset(&before, 0xAB, sizeof before);
    WArgs W = before;
    batch_settings(W, S, K, plan, P, ns, sched);
    const ll v[12] = {W.ns, W.group, W.shadow_node, W.chain, W.hybrid, W.cap, W.bucket, (ll)W.pool, (ll)W.level_cap,
                      W.child_sort, W.bucket_grid, W.pixel_major};
    memcpy(out, v, sizeof v);
    WArgs same = W;  // the words batch_settings may state, put back: the rest must be as it was
    same.ns = before.ns; same.group = before.group; same.shadow_node = before.shadow_node; same.chain = before.chain;
    same.hybrid = before.hybrid; same.cap = before.cap; same.bucket = before.bucket; same.pool = before.pool;
    same.level_cap = before.level_cap; same.child_sort = before.child_sort; same.bucket_grid = before.bucket_grid;
    same.pixel_major = before.pixel_major;
    ll changed = 0;
    for (size_t i = 0; i < sizeof same; ++i) changed += ((const unsigned char *)&same)[i] != ((const unsigned char *)&before)[i];
    out[12] = changed;
}

extern "C" ll bytes_per_path(ll profile, ll all_roots_prims, ll ns, ll max_depth, ll sched) {
    DScene S{};
    S.profile = (int32_t)profile;
    S.all_roots_prims = (int32_t)all_roots_prims;
    return (ll)pool_bytes_per_path(S, (int)ns, (int)max_depth, (int)sched);
}

// The pool a frame of `patches` patches x spp samples really reserves, default knobs: in {profile, all_roots_prims,
// max_children, patches, spp, ns, max_depth, max_paths}; out {paths of a batch, pool bytes, schedule}
extern "C" void real_pool(const ll *in, ll *out) {
    DScene S{};
    S.profile = (int32_t)in[0];
    S.all_roots_prims = (int32_t)in[1];
    S.max_children = (int32_t)in[2];
    RenderArgs A{};
    A.patches = (int32_t)in[3];
    A.spp = (int32_t)in[4];
    A.max_depth = (int32_t)in[6];
    const int ns = (int)in[5];
    const FrameKnobs K;
    const BatchPlan plan = plan_batches(S, A, ns, (size_t)in[7], K);
    const int sched = schedule_of(S, K);
    const size_t paths = (size_t)plan.npix * plan.nsb;
    const PoolShape P = pool_shape(sched, paths, std::max(1, A.max_depth), initial_pool_factor(sched, paths, K), ns, plan.persist, K);
    out[0] = (ll)paths;
    out[1] = (ll)pool_bytes(P.dims, fix_capacity(false, P.dims.rays, K));
    out[2] = sched;
}
