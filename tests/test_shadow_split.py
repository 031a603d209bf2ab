"""The node-per-lane shadow cast's split of a primitive's any-hit test into an origin side (the f32 local origin,
device_common.h prim_local_origin) and a direction side (prim_any_local), and of the root cull into root_slab +
root_needed_at, compiled for the host: the distance (accepted or not, as prim_any reads it) and the cull's
decision equal the unsplit forms' bit for bit.  Per root kind (Plane, Square, UnitBox, Sphere) a few hundred
thousand seeded rays through random similarity transforms: aimed at the primitive, starting ON its surface,
ending on it (t ~ 1), and with zero / negative-zero direction components."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "shadow_split_host.hip")
OUT = os.path.join(ROOT, "tests", "native", "_build", "libshadow_split_host.so")
HDRS = [os.path.join(ROOT, "jsraytracer_amd", "csrc", h) for h in ("device_common.h", "device_scene.h", "js_number.h", "fdlibm.h")]
PLANE, SQUARE, SPHERE, AABB = 1, 2, 4, 6  # include/jsrt_scene.h JSRT_GEOM_*


@pytest.fixture(scope="module")
def lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(f) for f in [SRC] + HDRS):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-fno-fast-math", "-fPIC", "-shared", SRC, "-o", OUT + f".{os.getpid()}.tmp"], check=True)
        os.replace(OUT + f".{os.getpid()}.tmp", OUT)
    L = ctypes.CDLL(OUT)
    P = ctypes.c_void_p
    L.split_any.argtypes = [P, P, P, P, ctypes.c_long, ctypes.c_double, ctypes.c_double, P, P]
    L.split_cull.argtypes = [P, P, ctypes.c_long, ctypes.c_double, ctypes.c_double, P, P]
    return L


def _cases(kind, seed, n=300_000):
    """World rays against one primitive kind under a random similarity transform (world = M local + c)."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    M = q * rng.uniform(0.2, 10, (n, 1, 1))
    c = rng.uniform(-5, 5, (n, 3))
    Minv = np.linalg.inv(M)
    inv = np.concatenate([Minv, (-Minv @ c[:, :, None])], 2).reshape(n, 12)
    box = np.concatenate([np.zeros((n, 3)), np.full((n, 3), 0.5)], 1).astype(np.float32)  # UnitBox
    # a local point on the primitive's surface
    loc = rng.uniform(-0.5, 0.5, (n, 3))
    if kind in (PLANE, SQUARE):
        loc[:, 2] = 0
        loc[:, :2] *= rng.choice([1.0, 2.4], (n, 1))  # inside and around the square's bounds
    elif kind == SPHERE:
        loc = rng.normal(size=(n, 3))
        loc /= np.linalg.norm(loc, axis=1, keepdims=True)
    else:
        ax = rng.integers(0, 3, n)
        loc[np.arange(n), ax] = rng.choice([-0.5, 0.5], n)
    target = ((M @ loc[:, :, None])[:, :, 0] + c).astype(np.float32).astype(np.float64)
    o = target + rng.normal(size=(n, 3)) * rng.uniform(0.1, 20, (n, 1))
    frac = rng.choice([0.3, 0.9, 1.0, 1.1, 3.0, 1e-4], n)
    d = (target - o) / frac[:, None]
    mode = rng.integers(0, 4, n)
    m = mode == 1  # the origin on the surface (a shadow ray leaving the primitive it was shaded on)
    o[m] = target[m]
    d[m] = rng.normal(size=(m.sum(), 3)) * rng.uniform(0.1, 10, (m.sum(), 1))
    m = mode == 2  # a zero / negative-zero direction component
    d[m, rng.integers(0, 3, m.sum())] = rng.choice([0.0, -0.0], m.sum())
    m = mode == 3  # axis-parallel world directions
    z = np.zeros((m.sum(), 3))
    z[np.arange(m.sum()), rng.integers(0, 3, m.sum())] = rng.choice([-1.0, 1.0], m.sum()) * rng.uniform(0.1, 10, m.sum())
    d[m] = z
    rays = np.concatenate([o, d], 1).astype(np.float32)
    return np.ascontiguousarray(inv), np.full(n, kind, np.int32), box, np.ascontiguousarray(rays)


@pytest.mark.parametrize("maxD", [1.0, np.inf])
@pytest.mark.parametrize("kind", [PLANE, SQUARE, AABB, SPHERE], ids=["plane", "square", "unitbox", "sphere"])
def test_split_distance_is_the_unsplit_one(lib, kind, maxD):
    inv, kinds, box, rays = _cases(kind, 20 + kind)
    n = len(kinds)
    a, b = np.empty(n), np.empty(n)
    lib.split_any(inv.ctypes.data, kinds.ctypes.data, box.ctypes.data, rays.ctypes.data, n, 1e-4, maxD,
                  a.ctypes.data, b.ctypes.data)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), np.flatnonzero(a.view(np.uint64) != b.view(np.uint64))[:8]
    acc = (a > 1e-4) & (a < maxD)
    assert acc.sum() > 1000 and (~acc).sum() > 1000  # both outcomes exercised


def test_split_cull_is_the_unsplit_one(lib):
    rng = np.random.default_rng(31)
    n = 400_000
    lo = rng.uniform(-5, 4, (n, 3))
    hi = lo + rng.uniform(0.01, 6, (n, 3))
    bounds = np.concatenate([lo, rng.uniform(0, 1e-3, (n, 1)), hi, rng.uniform(0, 1e-2, (n, 1))], 1).astype(np.float32)
    o = rng.uniform(-8, 8, (n, 3))
    d = rng.normal(size=(n, 3)) * rng.uniform(0.1, 20, (n, 1))
    z = rng.random(n) < 0.2
    d[z, rng.integers(0, 3, z.sum())] = rng.choice([0.0, -0.0], z.sum())  # rcp = +-inf: NaN slabs on a face
    onface = rng.random(n) < 0.2
    o[onface, 0] = lo[onface, 0]
    rays = np.ascontiguousarray(np.concatenate([o, d], 1).astype(np.float32))
    a, b = np.empty(n, np.int32), np.empty(n, np.int32)
    lib.split_cull(np.ascontiguousarray(bounds).ctypes.data, rays.ctypes.data, n, 1e-4, 1.0, a.ctypes.data, b.ctypes.data)
    assert np.array_equal(a, b)
    assert a.sum() > 1000 and (a == 0).sum() > 1000
