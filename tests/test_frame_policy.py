"""The frame driver's arithmetic (jsraytracer_amd/csrc/render_plan.h: the pool layout, pool_shape, initial_pool_factor,
level_bounds, batch_settings, learn_fractions, redo_step, pool_bytes_per_path), compiled for the host: what decides
whether a kernel writes past a buffer, which only GPU frames reached so far.

Every function is compared with a restatement, below, of the expressions run_frame and Wavefront::reserve held before
they moved (the `was_*` functions: written from that render.hip, not from the header), and checked for properties of
its own that a wrong restatement would not satisfy."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "frame_policy_host.hip")
OUT = os.path.join(ROOT, "tests", "native", "_build", "libframe_policy_host.so")
HDRS = [os.path.join(ROOT, "jsraytracer_amd", "csrc", h) for h in ("render_plan.h", "render_kernel.h", "device_scene.h")]
PF_ANALYTIC, PF_MESH, PF_SDF, PF_ALL = 0, 9, 4, 15  # device_scene.h
CHAIN, TREE, HYBRID = 0, 1, 2  # render_kernel.h SCHED_*
MAX_TREE_DEPTH, BKT_N, HAND_PLANES = 16, 64, 6
BKT_LEVEL = 3 * BKT_N * 16 + 64
LVL_UNDER, LVL_FLAG = 62, 63
# WArgs' buffers in the order Wavefront::reserve carved them, and their element sizes
NAMES = ["ox", "oy", "oz", "dx", "dy", "dz", "addr", "key", "t", "prim", "ctx", "path", "parent", "list0", "list1", "endl",
         "node", "child", "slot", "root", "hand", "hnode", "lvl", "qctr", "fixrec", "fixctr", "sray", "scol", "bkt", "bbase",
         "brank"]
ELEM = dict(ox=4, oy=4, oz=4, dx=4, dy=4, dz=4, addr=4, key=4, t=8, prim=4, ctx=4, path=4, parent=4, list0=4, list1=4,
            endl=1, node=16, child=16, slot=16, root=4, hand=16, hnode=4, lvl=4, qctr=4, fixrec=16, fixctr=4, sray=16,
            scol=16, bkt=4, bbase=4, brank=4)
KNOBS0 = (-1, 0, 0, 0)  # fix_cap unset, force_exact_pick, shadow_serial, pool_factor


def _ll(*v):
    return np.array(v, np.int64)


@pytest.fixture(scope="module")
def lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(f) for f in [SRC] + HDRS):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-fno-fast-math", "-fPIC", "-shared", SRC, "-o", OUT + f".{os.getpid()}.tmp"], check=True)
        os.replace(OUT + f".{os.getpid()}.tmp", OUT)
    L = ctypes.CDLL(OUT)
    P, LL, D = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_double
    for name, args in (("schedule", [LL] * 3), ("init_factor", [LL, LL, P]), ("shape", [LL] * 6 + [P, P]),
                       ("layout", [P, LL, P, P, P, P]), ("bounds", [LL] * 6 + [P, LL, LL, D, LL, P]),
                       ("redo", [P] + [LL] * 4), ("learn", [P, LL, P, LL, LL, LL]), ("settings", [P, P]),
                       ("bytes_per_path", [LL] * 5), ("real_pool", [P, P])):
        getattr(L, name).argtypes = args
        getattr(L, name).restype = LL
    return L


# ---- the layout -------------------------------------------------------------------------------------------------
def need(n, sz):
    return (n * sz + 255) & ~255


def was_fixcap(fix_all, rays, fix_cap, force):
    return rays + 4096 if fix_all else fix_cap if fix_cap >= 0 else rays + 4096 if force else rays // 8 + 4096


def was_reserve(rays, nodes, hands, paths, mode, shadow, fix_all, fix_cap, force):
    """Wavefront::reserve: its `bytes +=` list and, separately, its `carve` list -> (bytes, fixcap, {name: offset})."""
    tree, hybrid = mode == TREE, mode == HYBRID
    b = 8 * need(rays, 4) + need(rays, 8) + 2 * need(rays, 4)
    if tree:
        b += 2 * need(rays, 4)
    if hybrid:
        b += 3 * need(rays, 4) + need(rays, 1)
    b += need(nodes, 16) + need(4 * nodes, 16)
    if tree:
        b += need(2 * nodes, 16)
    if hybrid:
        b += need(nodes, 16)
    if tree or hybrid:
        b += need(3 * paths, 4)
    b += need(HAND_PLANES * hands, 16) + need(hands, 4) + need(64, 4)
    b += need(64, 4) + need(2 * shadow, 16) + need(shadow, 16)
    fixcap = was_fixcap(fix_all, rays, fix_cap, force)
    b += need(3 * fixcap, 16) + need(64, 4)
    if tree or hybrid:
        b += need(MAX_TREE_DEPTH * BKT_LEVEL, 4) + need((hands // 256 + 1) * BKT_N, 4) + need(rays, 4)
    carve = [(n, rays) for n in NAMES[:11]]
    if tree:
        carve += [("path", rays), ("parent", rays)]
    if hybrid:
        carve += [("parent", rays), ("list0", rays), ("list1", rays), ("endl", rays)]
    carve += [("node", nodes), ("child", 4 * nodes)]
    if tree:
        carve += [("slot", 2 * nodes)]
    if hybrid:
        carve += [("slot", nodes)]
    if tree or hybrid:
        carve += [("root", 3 * paths)]
    carve += [("hand", HAND_PLANES * hands), ("hnode", hands), ("lvl", 64), ("qctr", 64), ("fixrec", 3 * fixcap), ("fixctr", 64)]
    if shadow:
        carve += [("sray", 2 * shadow), ("scol", shadow)]
    if tree or hybrid:
        carve += [("bkt", MAX_TREE_DEPTH * BKT_LEVEL), ("bbase", (hands // 256 + 1) * BKT_N), ("brank", rays)]
    off, p = {}, 0
    for name, n in carve:
        off[name] = p
        p += need(n, ELEM[name])
    return b, fixcap, off


USED = {CHAIN: set(NAMES) - {"path", "parent", "list0", "list1", "endl", "slot", "root", "bkt", "bbase", "brank"},
        TREE: set(NAMES) - {"list0", "list1", "endl"}, HYBRID: set(NAMES) - {"path"}}


def test_layout_is_the_reserve_it_replaces(lib):
    n = 0
    for mode, rays, depth, shadowed, fix_all, fix_cap, force in itertools.product(
            (CHAIN, TREE, HYBRID), (64, 256, 1000, 4096, 2**20 + 64), (1, 8, 16), (0, 1), (0, 1), (-1, 0, 7), (0, 1)):
        nodes, hands, paths = rays * depth, rays, max(1, rays // 3)
        shadow = hands * 4 if shadowed else 0
        head, off, size = np.empty(7, np.int64), np.empty(31, np.int64), np.empty(31, np.int64)
        d, k = _ll(rays, nodes, hands, paths, mode, shadow), _ll(fix_cap, force, 0, 0)
        lib.layout(d.ctypes.data, fix_all, k.ctypes.data, head.ctypes.data, off.ctypes.data, size.ctypes.data)
        total, fixcap = int(head[0]), int(head[1])
        case = (mode, rays, depth, shadow, fix_all, fix_cap, force)
        present = [(int(off[i]), int(size[i]), NAMES[i]) for i in range(31) if off[i] >= 0]
        # properties of the layout itself
        assert all(o % 256 == 0 for o, _, _ in present), case
        assert [nm for _, _, nm in present] == [nm for _, _, nm in sorted(present)], case  # the carve order
        for (o, s, nm), (o2, _, _) in zip(present, present[1:]):
            assert o + s <= o2, (case, nm)  # disjoint
        assert present[0][0] == 0 and need(present[-1][1], 1) + present[-1][0] == total, case
        want = USED[mode] - (set() if shadow else {"sray", "scol"})
        assert {nm for _, _, nm in present} == want, case  # what the mode does not use is null
        assert all(size[i] == 0 for i in range(31) if off[i] < 0), case
        assert head[6] == 0, case  # carve_pool leaves the other words zero
        # ... and the parent's
        wb, wfix, woff = was_reserve(rays, nodes, hands, paths, mode, shadow, fix_all, fix_cap, force)
        assert (total, fixcap) == (wb, wfix), case
        assert {nm: o for o, _, nm in present} == woff, case
        assert list(head[2:6]) == [wfix, nodes, hands, shadow], case  # fixcap, nstride, hstride, sstride
        n += 1
    assert n == 3 * 5 * 3 * 2 * 2 * 3 * 2


# ---- pool_shape, initial_pool_factor ------------------------------------------------------------------------------
def was_shape(sched, paths, depth, factor, ns, persist, shadow_serial):
    hybrid, chain = sched == HYBRID, sched != TREE
    cap = ((paths + paths * factor // 4 + 255) & ~255) if hybrid else paths
    fits = not (hybrid and cap * depth >= 1 << 32)
    pool = cap if chain else paths * factor
    level_cap = cap if chain else pool // 2
    group = 1
    if 1 < ns <= 64 and not (shadow_serial and not persist):
        while group < ns:
            group *= 2
    hands = cap if chain else max(level_cap, paths)
    shadow = hands * group if persist else 0
    dims = [cap, cap * depth, cap, paths, sched, shadow] if chain else [pool, pool, hands, paths, TREE, shadow]
    return [cap, pool, level_cap, group, hands, shadow, int(fits)] + dims


def _shape(lib, sched, paths, depth, factor, ns, persist, serial):
    out, k = np.empty(13, np.int64), _ll(-1, 0, serial, 0)
    lib.shape(sched, paths, depth, factor, ns, persist, k.ctypes.data, out.ctypes.data)
    return [int(x) for x in out]


def test_pool_shape(lib):
    fits = set()
    for sched, paths, depth, factor, ns, persist, serial in itertools.product(
            (CHAIN, TREE, HYBRID), (64, 4096, 2**20, 2**20 + 64, 2**25), (1, 8, 16), (1, 2, 8, 16), (0, 1, 2, 4, 5, 64, 65),
            (0, 1), (0, 1)):
        got = _shape(lib, sched, paths, depth, factor, ns, persist, serial)
        case = (sched, paths, depth, factor, ns, persist, serial)
        assert got == was_shape(*case), case
        cap, pool, level_cap, group, hands, shadow, fit = got[:7]
        if serial and not persist:
            assert group == 1, case
        else:
            assert group == (1 << (ns - 1).bit_length() if 2 <= ns <= 64 else 1), case  # least power of two >= ns
        assert bool(fit) == (sched != HYBRID or cap * depth < 2**32), case
        assert cap >= paths and hands >= min(level_cap, paths) and shadow == (hands * group if persist else 0), case
        fits.add((sched, fit))
    # the edge: cap x depth = 2^32 exactly does not fit (a u32 node index), one 256-slot step below does
    for paths, factor, depth, want in ((2**27, 4, 16, 0), (2**27 - 128, 4, 16, 1), (2**28, 4, 8, 0), (2**28 - 128, 4, 8, 1),
                                       (2**25, 16, 16, 1), (2**26, 16, 16, 0)):
        got = _shape(lib, HYBRID, paths, depth, factor, 1, 0, 0)
        assert got == was_shape(HYBRID, paths, depth, factor, 1, 0, 0)
        assert got[6] == want and (got[0] * depth < 2**32) == bool(want), (paths, factor, depth, got[0] * depth)
        assert _shape(lib, TREE, paths, depth, factor, 1, 0, 0)[6] == 1  # only the hybrid chain indexes nodes so
    assert _shape(lib, HYBRID, 2**27, 16, 4, 1, 0, 0)[0] * 16 == 2**32


def test_initial_pool_factor(lib):
    for sched, paths, knob in itertools.product((TREE, HYBRID), (64, 4096, 2**20, 2**20 + 64, 2**25), (0, 1, 3)):
        k = _ll(-1, 0, 0, knob)
        was = knob if knob else ((8 if paths <= 1 << 20 else 2) if sched == HYBRID else 8)
        assert lib.init_factor(sched, paths, k.ctypes.data) == was, (sched, paths, knob)


def test_schedule_of(lib):
    for mc, pf, knob in itertools.product((0, 1, 2), (PF_ANALYTIC, PF_MESH, PF_SDF, PF_ALL), (-1, 0, 1)):
        was = CHAIN if mc <= 1 else (HYBRID if knob else TREE) if knob >= 0 else HYBRID if pf == PF_ANALYTIC else TREE
        assert lib.schedule(mc, pf, knob) == was, (mc, pf, knob)


# ---- level_bounds -----------------------------------------------------------------------------------------------
def was_bounds(sched, np_, cap, level_cap, max_depth, max_children, frac, conservative, margin, slack):
    b = [0] * max(1, max_depth)
    if sched == HYBRID:
        for L in range(max_depth):
            b[L] = np_ if L == 0 else cap
            if L > 0 and not conservative and L < len(frac):
                b[L] = min(cap, max(256, int(float(np_) * frac[L] * margin) + slack))
        return b
    ub = np_
    for L in range(max_depth):
        if ub <= 0:
            break
        b[L] = ub
        if not conservative and L < len(frac):
            b[L] = min(ub, max(256, int(float(np_) * frac[L] * margin) + slack))
        ub = min(ub * max_children, level_cap) if L + 1 < max_depth else 0
    return b


def _bounds(lib, sched, np_, paths, max_depth, factor, mc, frac, conservative, margin, slack):
    f = np.array(frac, np.float64)
    out = np.full(max(1, max_depth), -1, np.int64)
    n = lib.bounds(sched, np_, paths, max_depth, factor, mc, f.ctypes.data, len(frac), conservative, margin, slack, out.ctypes.data)
    assert n == len(out)
    return [int(x) for x in out]


def test_level_bounds(lib):
    fracs = ([], [1.0, 0.5, 0.0], [1.0, 0.9, 0.8, 0.7, 1e-7, 0.0, 0.3, 0.2], [1.0] + [3.0] * 15)
    for sched, (paths, np_), max_depth, factor, mc, frac, conservative, (margin, slack) in itertools.product(
            (TREE, HYBRID), ((4096, 4096), (4096, 1000), (2**20 + 64, 2**20 + 64), (64, 64)), (0, 1, 4, 8, 16), (1, 8), (0, 1, 2),
            fracs, (0, 1), ((1.25, 4096), (1.0, 0), (0.5, 0))):
        case = (sched, paths, np_, max_depth, factor, mc, frac, conservative, margin, slack)
        cap, pool, level_cap = was_shape(sched, paths, max(1, max_depth), factor, 0, 0, 0)[:3]
        got = _bounds(lib, sched, np_, paths, max_depth, factor, mc, frac, conservative, margin, slack)
        was = was_bounds(sched, np_, cap, level_cap, max_depth, mc, frac, conservative, margin, slack)
        assert got == was, case
        # level 0 is the batch's paths (a tree's learned frac[0] is 1: only a margin below 1 can lower it)
        if max_depth >= 1 and (sched == HYBRID or not frac or conservative or margin >= 1):
            assert got[0] == np_, case
        # conservative bounds do not read frac
        assert _bounds(lib, sched, np_, paths, max_depth, factor, mc, frac, 1, margin, slack) == \
            _bounds(lib, sched, np_, paths, max_depth, factor, mc, [], 1, 7.0, 3), case
        if sched == HYBRID:
            assert all(x <= cap for x in got[1:]), case
            if not conservative:  # learned: at least one block, even at a learned count of 0
                assert all(got[L] >= min(256, cap) for L in range(1, min(len(frac), max_depth))), case
        else:
            ub, dead = np_, False
            for L in range(max_depth):
                dead = dead or ub == 0
                assert got[L] <= ub and (not dead or got[L] == 0), (case, L)  # 0 from the first level whose ub is 0
                if not dead and not conservative and L < len(frac):
                    assert got[L] >= min(256, ub), (case, L)
                ub = min(ub * mc, level_cap) if L + 1 < max_depth else 0
    # the first level of a tree batch is np paths whatever was learned above it (frac[0] = 1 with any margin >= 1)
    assert _bounds(lib, TREE, 4096, 4096, 4, 8, 2, [1.0, 2.0], 0, 1.25, 4096)[0] == 4096
    # JSRT_BOUND_MARGIN's pair: margin x count, no slack -- a tight margin under the learned count, the default above it
    assert _bounds(lib, TREE, 10000, 10000, 3, 8, 2, [1.0, 0.5, 0.25], 0, 1.0, 0) == [10000, 5000, 2500]
    assert _bounds(lib, TREE, 10000, 10000, 3, 8, 2, [1.0, 0.5, 0.25], 0, 0.5, 0) == [5000, 2500, 1250]
    assert _bounds(lib, TREE, 10000, 10000, 3, 8, 2, [1.0, 0.5, 0.25], 0, 1.25, 4096) == [10000, 10346, 7221]
    assert _bounds(lib, HYBRID, 10000, 10000, 3, 8, 2, [1.0, 0.5, 0.25], 0, 1.25, 4096) == [10000, 10346, 7221]


def test_learn_fractions(lib):
    def learn(frac, lvl, max_depth, hybrid, npaths):
        f = np.zeros(max(len(frac), max_depth), np.float64)
        f[:len(frac)] = frac
        lv = np.zeros(64, np.uint32)
        for k, v in lvl.items():
            lv[k] = v
        n = lib.learn(f.ctypes.data, len(frac), lv.ctypes.data, max_depth, hybrid, npaths)
        return list(f[:n])
    assert learn([], {0: 1000, 1: 500, 2: 10}, 3, 0, 1000) == [1.0, 0.5, 0.01]
    assert learn([1.0, 0.75, 0.0], {0: 1000, 1: 500, 2: 10}, 3, 0, 1000) == [1.0, 0.75, 0.01]  # the maximum over batches
    assert learn([], {0: 1000, 1: 0, 2: 400, 3: 100, 4: 1, 5: 2}, 3, 1, 1000) == [1.0, 0.5, 0.003]  # pairs {continuing, started}
    for flag in (LVL_FLAG, LVL_UNDER):  # a poisoned batch teaches nothing
        assert learn([], {0: 1000, 1: 500, flag: 1}, 2, 0, 1000) == []
        assert learn([1.0, 0.25], {0: 1000, 1: 500, flag: 1}, 2, 0, 1000) == [1.0, 0.25]


# ---- the depth limits: maxRecursionDepth 1 and MAX_TREE_DEPTH ---------------------------------------------------
def test_level_bounds_at_depth_1_and_16(lib):
    """One level: a single entry, the batch's paths.  Sixteen: sixteen entries, the last one from frac[15] (learned) or
    the level's most (conservative) -- a table one entry short, or a loop that stops at 15, shows here alone."""
    for sched, frac, conservative in itertools.product((TREE, HYBRID), ([], [1.0], [1.0] + [0.5] * 15), (0, 1)):
        assert _bounds(lib, sched, 768, 768, 1, 8, 2, frac, conservative, 1.25, 4096) == [768], (sched, frac, conservative)
    np_ = 100000
    frac = [1.0] + [(L + 1) / 100 for L in range(1, MAX_TREE_DEPTH)]  # a value per level: 2 %, 3 %, ... 16 %
    want = [np_] + [1000 * (L + 1) for L in range(1, MAX_TREE_DEPTH)]
    for sched in (TREE, HYBRID):
        assert _bounds(lib, sched, np_, np_, 16, 8, 2, frac, 0, 1.0, 0) == want, sched
        assert _bounds(lib, sched, np_, np_, 16, 8, 2, frac + [0.9, 0.9], 0, 1.0, 0) == want, sched  # no 17th level
    # conservative: the hybrid chain's 15 deeper levels may hold every chain slot; the tree's double up to level_cap
    cap, pool, level_cap = was_shape(HYBRID, 768, 16, 8, 0, 0, 0)[:3]
    assert cap == 2304 and _bounds(lib, HYBRID, 768, 768, 16, 8, 2, [], 0, 1.25, 4096) == [768] + [cap] * 15
    cap, pool, level_cap = was_shape(TREE, 768, 16, 8, 0, 0, 0)[:3]
    assert level_cap == 3072
    assert _bounds(lib, TREE, 768, 768, 16, 8, 2, [], 0, 1.25, 4096) == [768, 1536] + [3072] * 14
    assert _bounds(lib, TREE, 768, 768, 16, 8, 1, [], 0, 1.25, 4096) == [768] * 16
    # counts learned by a frame of depth 8 bound the first 8 levels of a frame of depth 16, the rest are conservative
    got = _bounds(lib, HYBRID, np_, np_, 16, 8, 2, frac[:8], 0, 1.0, 0)
    assert got[:8] == want[:8] and got[8:] == [was_shape(HYBRID, np_, 16, 8, 0, 0, 0)[0]] * 8


def test_learn_fractions_at_depth_1_and_16(lib):
    def learn(frac, lvl, max_depth, hybrid, npaths):
        f = np.zeros(max(len(frac), max_depth), np.float64)
        f[:len(frac)] = frac
        lv = np.zeros(64, np.uint32)
        for k, v in lvl.items():
            lv[k] = v
        n = lib.learn(f.ctypes.data, len(frac), lv.ctypes.data, max_depth, hybrid, npaths)
        return list(f[:n])
    # one level: one entry, whatever the words beyond it hold
    assert learn([], {0: 1000, 1: 7, 2: 7}, 1, 0, 1000) == [1.0]
    assert learn([], {0: 1000, 1: 0, 2: 7, 3: 7}, 1, 1, 1000) == [1.0]
    assert learn([0.5], {0: 250}, 1, 0, 1000) == [0.5]
    # sixteen levels: lvl[15] (tree), the pair lvl[30, 31] (hybrid chain) are the last words read -- below the frame
    # flags lvl[62, 63] -- and the words after them are not
    tree = {L: 1000 - 50 * L for L in range(MAX_TREE_DEPTH)}
    assert learn([], {**tree, 16: 999999}, 16, 0, 1000) == [(1000 - 50 * L) / 1000 for L in range(16)]
    pairs = {}
    for L in range(MAX_TREE_DEPTH):
        pairs[2 * L], pairs[2 * L + 1] = 800 - 40 * L, 3 * L
    assert 2 * (MAX_TREE_DEPTH - 1) + 1 < LVL_UNDER
    want = [(800 - 40 * L + 3 * L) / 1000 for L in range(16)]
    assert want[15] == (200 + 45) / 1000
    assert learn([], {**pairs, 32: 999999, 33: 999999}, 16, 1, 1000) == want
    assert learn([1.0] * 16, pairs, 16, 1, 1000) == [1.0] * 16  # the maximum over batches, level by level
    for flag in (LVL_FLAG, LVL_UNDER):
        assert learn([], {**pairs, flag: 1}, 16, 1, 1000) == []


# the batches of the thumbnail frames of tests/test_gpu_frames.py: (patches, spp) of 1 x 1 and 1 x 7 (one patch),
# 20 x 12 (6), 37 x 23 (15) and 9 x 65 (18 patches)
FRAMES = [(1, 1), (1, 3), (6, 2), (15, 1), (15, 3), (18, 3)]


def test_pool_carve_of_the_smallest_frames(lib):
    """A one-patch batch at depths 1 and 16, and the thumbnails' batches, on every schedule and at the first pool
    factors a frame can start from: the pool holds the tables the depth indexes -- depth x cap node records (chain
    layouts), MAX_TREE_DEPTH bucket levels, 64 level words -- disjoint, within its size."""
    for (patches, spp), depth, sched, factor in itertools.product(FRAMES, (1, 16), (CHAIN, TREE, HYBRID), (1, 8)):
        paths = patches * 64 * spp
        shp = _shape(lib, sched, paths, depth, factor, 4, 0, 0)
        assert shp == was_shape(sched, paths, depth, factor, 4, 0, 0)
        cap, pool, level_cap, group, hands, shadow, fits = shp[:7]
        dims = shp[7:]
        head, off, size = np.empty(7, np.int64), np.empty(31, np.int64), np.empty(31, np.int64)
        lib.layout(_ll(*dims).ctypes.data, 0, _ll(*KNOBS0).ctypes.data, head.ctypes.data, off.ctypes.data, size.ctypes.data)
        case = (patches, spp, depth, sched, factor)
        at = {NAMES[i]: (int(off[i]), int(size[i])) for i in range(31) if off[i] >= 0}
        assert fits and cap >= paths, case
        if sched == TREE:
            assert at["node"][1] == 16 * pool and at["slot"][1] == 2 * 16 * pool and pool == paths * factor, case
        else:
            assert at["node"][1] == 16 * cap * depth and at["child"][1] == 4 * 16 * cap * depth, case  # node [L * cap + slot]
            assert int(head[3]) == cap * depth, case  # nstride
        if sched == HYBRID:
            assert at["slot"][1] == 16 * cap * depth and at["endl"][1] == cap and cap % 256 == 0, case
        if sched != CHAIN:
            assert at["bkt"][1] == 4 * MAX_TREE_DEPTH * BKT_LEVEL and at["root"][1] == 4 * 3 * paths, case
        assert at["lvl"][1] == 4 * 64 and at["qctr"][1] == 4 * 64, case
        assert 2 * depth <= LVL_UNDER and 32 + depth <= 64, case  # count pairs below the flags; qctr [L], [32 + L]
        spans = sorted(at.values())
        assert all(o + s <= o2 for (o, s), (o2, _) in zip(spans, spans[1:])), case
        assert spans[-1][0] + spans[-1][1] <= int(head[0]), case
        # the launch bounds of such a batch never ask a level for more than the pool gives it
        b = _bounds(lib, sched, paths, paths, depth, factor, 2, [], 1, 1.25, 4096) if sched != CHAIN else []
        assert len(b) == (depth if sched != CHAIN else 0) and all(x <= (cap if sched == HYBRID else max(paths, level_cap)) for x in b), case


# ---- redo_step --------------------------------------------------------------------------------------------------
def _redo(lib, factor, fix_all, twin, twin_fix, nfrac, conservative, sched, paths, flag, under):
    st = _ll(factor, fix_all, twin, twin_fix, nfrac, conservative)
    r = lib.redo(st.ctypes.data, sched, paths, flag, under)
    return int(r), [int(x) for x in st]


def test_redo_step_decision_table(lib):
    # chain: the first overflow sets fix_all on both pools, the second is out of memory
    assert _redo(lib, 8, 0, 1, 0, 3, 0, CHAIN, 4096, 1, 0) == (0, [8, 1, 1, 1, 3, 0])
    assert _redo(lib, 8, 1, 1, 1, 3, 0, CHAIN, 4096, 1, 0) == (1, [8, 1, 1, 1, 3, 0])
    assert _redo(lib, 8, 0, 0, 0, 3, 0, CHAIN, 4096, 1, 0) == (0, [8, 1, 0, 0, 3, 0])  # no twin pool
    assert _redo(lib, 8, 1, 0, 0, 3, 0, CHAIN, 4096, 1, 0) == (1, [8, 1, 0, 0, 3, 0])
    assert _redo(lib, 8, 1, 1, 0, 3, 0, CHAIN, 4096, 1, 0) == (0, [8, 1, 1, 1, 3, 0])  # a twin made after the first redo
    for sched, under in itertools.product((TREE, HYBRID), (0, 1)):
        # LVL_FLAG, with or without LVL_UNDER: twice the pool, frac cleared, the bounds stay as they were
        assert _redo(lib, 8, 0, 1, 0, 3, 0, sched, 4096, 1, under) == (0, [16, 0, 1, 0, 0, 0])
        assert _redo(lib, 2, 0, 0, 0, 3, 1, sched, 4096, 1, under) == (0, [4, 0, 0, 0, 0, 1])
        # ... out of memory past 2^31 x (hybrid ? 4 : 1) pool slots
        limit = 2**31 * (4 if sched == HYBRID else 1)
        assert _redo(lib, 8, 0, 0, 0, 3, 0, sched, limit // 8, 1, under) == (0, [16, 0, 0, 0, 0, 0])
        assert _redo(lib, 8, 0, 0, 0, 3, 0, sched, limit // 8 + 1, 1, under) == (1, [8, 0, 0, 0, 3, 0])
    for sched in (TREE, HYBRID):  # LVL_UNDER alone: conservative bounds, frac cleared, the pool stays
        assert _redo(lib, 8, 0, 1, 0, 3, 0, sched, 4096, 0, 1) == (0, [8, 0, 1, 0, 0, 1])
    # a frame that is poisoned whatever the pool ends: within the doublings the limit allows
    for sched, paths in itertools.product((TREE, HYBRID), (64, 4096, 2**20 + 64, 2**25)):
        st, n = [8, 0, 1, 0, 3, 0], 0
        while True:
            r, st = _redo(lib, *st, sched, paths, 1, 0)
            if r:
                break
            n += 1
            assert n <= 40
        limit = 2**31 * (4 if sched == HYBRID else 1)
        assert paths * st[0] > limit >= paths * st[0] // 2 and st[0] == 8 << n, (sched, paths, st, n)
    st, n = [8, 0, 1, 0, 3, 0], 0
    while not (r := _redo(lib, *st, CHAIN, 4096, 1, 0))[0]:
        st, n = r[1], n + 1
    assert n == 1


# ---- batch_settings ---------------------------------------------------------------------------------------------
def test_batch_settings(lib):
    for pf, n_prims, grid_cells, sched, persist, pm, ns, shadow_node, bucket, child_sort, bucket_grid in itertools.product(
            (PF_ANALYTIC, PF_MESH, PF_SDF), (0, 1, 64, 65, 4096, 100000), (0, 27), (CHAIN, TREE, HYBRID), (0, 1), (0, 1),
            (0, 1, 4, 64, 65), (0, 1), (0, 1), (-1, 0, 1), (-1, 0, 1)):
        paths, depth, factor = 4096, 8, 8
        out = np.empty(13, np.int64)
        lib.settings(_ll(pf, n_prims, grid_cells, sched, persist, pm, ns, paths, depth, factor, shadow_node, bucket, child_sort,
                         bucket_grid).ctypes.data, out.ctypes.data)
        got = dict(zip("ns group shadow_node chain hybrid cap bucket pool level_cap child_sort bucket_grid pixel_major changed".split(),
                       (int(x) for x in out)))
        case = (pf, n_prims, grid_cells, sched, persist, pm, ns, shadow_node, bucket, child_sort, bucket_grid)
        shp = was_shape(sched, paths, depth, factor, ns, persist, 0)
        # the parent's `settings` lambda
        shift = 0
        while n_prims > 0 and ((n_prims - 1) >> shift) >= BKT_N:
            shift += 1
        learned, chain = sched != CHAIN, sched != TREE
        was_bucket = shift + 1 if (learned and not persist and n_prims > 0 and 0 < ns <= 64 and bucket) else 0
        grid = bucket_grid == 1 if bucket_grid >= 0 else pf == PF_ANALYTIC
        was = dict(ns=ns, group=shp[3], shadow_node=shadow_node, chain=int(chain), hybrid=int(sched == HYBRID), cap=shp[0],
                   bucket=was_bucket, pool=shp[1], level_cap=shp[2],
                   child_sort=int(not chain and (child_sort == 1 if child_sort >= 0 else (pf & 1) != 0)),
                   bucket_grid=int(bool(was_bucket) and grid_cells > 0 and grid), pixel_major=pm, changed=0)
        assert got == was, case  # changed = 0: every pointer, stride and batch word is left alone
        # properties
        if got["bucket"]:
            s = got["bucket"] - 1
            assert (n_prims - 1) >> s < 64 and (s == 0 or (n_prims - 1) >> (s - 1) >= 64), case  # the least shift
        if persist or ns == 0 or ns > 64 or sched == CHAIN or not bucket or n_prims == 0:
            assert got["bucket"] == 0, case
        else:
            assert got["bucket"] >= 1, case
        assert not got["child_sort"] or sched == TREE, case
        assert not got["bucket_grid"] or (got["bucket"] and grid_cells > 0), case


# ---- pool_bytes_per_path ----------------------------------------------------------------------------------------
def was_bytes_per_path(pf, all_roots_prims, ns, max_depth, sched):
    ray, node, hand = 8 * 4 + 8 + 2 * 4, 16 + 4 * 16, HAND_PLANES * 16 + 4
    persist = bool(pf & PF_SDF) and bool(all_roots_prims)
    group = 1
    while group < ns and ns <= 64:
        group *= 2
    depth = max(1, max_depth)
    q = group * 48 if persist else 0
    if sched == CHAIN:
        return ray + depth * node + hand + q
    if sched == HYBRID:
        return (4 + 2) * (ray + 17 + depth * (node + 16) + hand + q + BKT_N * 4 // 256) // 4 + 12
    pool, level_cap = 8, 4
    return pool * (ray + 8 + node + 2 * 16 + 4) + level_cap * (hand + q + BKT_N * 4 // 256) + 12


def test_bytes_per_path_keeps_its_values(lib):
    for pf, arp, ns, depth, sched in itertools.product((PF_ANALYTIC, PF_MESH, PF_SDF, PF_ALL), (0, 1), (0, 1, 2, 4, 5, 64, 65),
                                                       (0, 1, 8, 16), (CHAIN, TREE, HYBRID)):
        assert lib.bytes_per_path(pf, arp, ns, depth, sched) == was_bytes_per_path(pf, arp, ns, depth, sched), (pf, arp, ns, depth, sched)
    assert lib.bytes_per_path(PF_MESH, 0, 1, 4, TREE) == 8 * 172 + 4 * 101 + 12  # the "about 1.8 KB per path" of the tree


# The four benchmark frames (bench.py CONFIGS) at the default batch of 2^25 paths: {profile, all_roots_prims, patches,
# spp, light samples, max_depth}; every one of them branches (max_children 2).
BENCH = {"cornell_box_path (hybrid chain, depth 8)": (PF_ANALYTIC, 1, 128 * 128, 64, 4, 8),
         "bunny (tree)": (PF_MESH, 0, 240 * 135, 16, 2, 4),
         "SDF_Menger (tree, persistent casts)": (PF_SDF, 1, 128 * 128, 32, 1, 4),
         "dragon (tree)": (PF_MESH, 0, 512 * 512, 256, 1, 4)}


def test_bytes_per_path_beside_the_real_layout(lib, capsys):
    """The estimate that caps the default batch beside what such a batch reserves (printed; DESIGN.md §3 quotes it).
    Nothing is asserted about their ratio: the estimate's values are pinned above, the real figure by the layout test."""
    with capsys.disabled():
        print()
        for name, (pf, arp, patches, spp, ns, depth) in BENCH.items():
            out = np.empty(3, np.int64)
            lib.real_pool(_ll(pf, arp, 2, patches, spp, ns, depth, 2**25).ctypes.data, out.ctypes.data)
            paths, nbytes, sched = (int(x) for x in out)
            est = lib.bytes_per_path(pf, arp, ns, depth, sched)
            print(f"  {name}: batch of {paths} paths, {nbytes / paths:.1f} B/path reserved, estimate {est} B/path")
            assert paths > 0 and nbytes > 0
