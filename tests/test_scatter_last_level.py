"""k_shade's last level shades its nodes without their child directions (shade_node<NODIR>, device_common.h
scatter_children<true> / path_scatter<true>): the children are black without a cast, and the resolve reads only
their count and their factors col, w, k.  Compiled for the host, the two forms of the scatter are compared on
constructed hits, per material kind (Phong, Fresnel, path tracing): the child count, each child's col, w and k, and
the RNG call count the node's frame ends on, all bit for bit.  120 K hits per kind and mirror probability: kr at 0,
at 1, just inside both and in between; normals at grazing angles to the view direction (V . N = 0, 1e-9, 1e-4);
absorbed draws (diffusivity and specularity both black: probSum = 0; a refraction side without a refracted
direction); black and unit reflectivity / transmissivity; every diffuse pick through the fix path (force_fix)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "scatter_nodir_host.hip")
OUT = os.path.join(ROOT, "tests", "native", "_build", "libscatter_nodir_host.so")
HDRS = [os.path.join(ROOT, "jsraytracer_amd", "csrc", h) for h in ("device_common.h", "device_scene.h", "js_number.h", "fdlibm.h")]
PHONG, FRESNEL, PATH = 1, 2, 3  # include/jsrt_scene.h JSRT_MAT_*
N = 120_000


@pytest.fixture(scope="module")
def lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(f) for f in [SRC] + HDRS):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-fno-fast-math", "-fPIC", "-shared", SRC, "-o", OUT + f".{os.getpid()}.tmp"], check=True)
        os.replace(OUT + f".{os.getpid()}.tmp", OUT)
    L = ctypes.CDLL(OUT)
    P = ctypes.c_void_p
    L.scatter_both.argtypes = [P, ctypes.c_long, ctypes.c_int, ctypes.c_double, ctypes.c_int, P, P]
    return L


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _hits(seed, n=N):
    rng = np.random.default_rng(seed)
    V = _unit(rng.normal(size=(n, 3)))
    Nn = _unit(rng.normal(size=(n, 3)))
    g = rng.random(n) < 0.3  # grazing: N perpendicular to V up to a small tilt toward it
    perp = _unit(np.cross(V[g], rng.normal(size=(g.sum(), 3))))
    Nn[g] = _unit(perp + rng.choice([0.0, 1e-9, 1e-4], (g.sum(), 1)) * V[g])
    vdotn = (V * Nn).sum(1, keepdims=True)
    Nn = np.where(vdotn < 0, -Nn, Nn)
    vdotn = np.abs(vdotn)
    R = _unit(2 * vdotn * Nn - V)
    refr = rng.normal(size=(n, 3))
    col = lambda: rng.uniform(0, 1, (n, 3)) * rng.choice([0.0, 1.0, 1.0, 1.0], (n, 1))  # a quarter black
    diff, spec, refl, trans = col(), col(), col(), col()
    unit = rng.random(n) < 0.2
    refl[unit] = 1.0
    trans[rng.random(n) < 0.2] = 1.0
    kr = rng.choice([0.0, 1.0, 1e-12, 1 - 1e-12, 0.5], n) * 1.0
    mid = kr == 0.5
    kr[mid] = rng.uniform(0, 1, mid.sum())
    x = np.concatenate([Nn, R, refr, diff, spec, refl, trans, kr[:, None], (rng.random(n) < 0.7)[:, None].astype(float),
                        -V * rng.uniform(0.1, 5, (n, 1)), rng.integers(0, 2**32, (n, 1)).astype(float),
                        rng.integers(0, 2**32, (n, 1)).astype(float), rng.integers(0, 9, (n, 1)).astype(float)], 1)
    assert x.shape[1] == 29
    return np.ascontiguousarray(x)


# (the mirror probability and the pick's fix are read by the path-tracing scatter only)
CASES = [(PHONG, 0.3, 0), (FRESNEL, 0.3, 0)] + [(PATH, m, f) for m in (0.0, 0.3, 1.0) for f in (0, 1)]


@pytest.mark.parametrize("kind,mirror,force", CASES,
                         ids=[f"{ {PHONG: 'phong', FRESNEL: 'fresnel', PATH: 'path'}[k]}_mirror{m}_{'forced_fix' if f else 'picks'}" for k, m, f in CASES])
def test_children_without_directions_are_the_full_ones(lib, kind, mirror, force):
    x = _hits(100 * kind + int(10 * mirror))
    out = np.full((N, 2, 17), 0xDEADBEEF, np.uint32)
    calls = np.zeros((N, 2), np.uint32)
    lib.scatter_both(x.ctypes.data, N, kind, mirror, force, out.ctypes.data, calls.ctypes.data)
    full, nodir = out[:, 0], out[:, 1]
    bad = np.flatnonzero((full != nodir).any(1))
    assert bad.size == 0, (bad[:8], full[bad[:2]], nodir[bad[:2]])
    assert np.array_equal(calls[:, 0], calls[:, 1])  # the refraction side drew the same numbers
    n = full[:, 0]
    assert set(np.unique(n)) == {0, 1, 2} and min((n == k).sum() for k in (0, 1, 2)) > 1000  # every count exercised
    if kind == PATH and 0 < mirror < 1:
        drawn = calls[:, 0] - x[:, 28].astype(np.uint32)
        assert {1, 2, 4} <= set(np.unique(drawn))  # mirror (1 draw), specular / absorbed (2), a diffuse pick (4)
