"""PositionalUVMaterial's mapping (jsraytracer_amd/csrc/posuv_map.h posuv_map), compiled for the host, against the
reference's own PositionalUVMaterial.color (materials.js:188-191): fed the data.position of every recorded hit under
a wrapper (tests/golden/posuv/, tools/make_posuv_fixtures.js), it returns the data.UV the base material received, bit
for bit.  Constructed cases pin the numeric model -- delta an f32 Vec, the dot product f64 products summed left to
right and rounded once -- where a sloppier one (f32 accumulation, a fused multiply-add) gives another f32."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import posuv_kats as pk

SRC = os.path.join(pk.ROOT, "tests", "native", "posuv_map_host.hip")
OUT = os.path.join(pk.ROOT, "tests", "native", "_build", "libposuv_map_host.so")
HDRS = [os.path.join(pk.ROOT, "jsraytracer_amd", "csrc", "posuv_map.h"), os.path.join(pk.ROOT, "include", "jsrt_scene.h")]


@pytest.fixture(scope="module")
def lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(f) for f in [SRC] + HDRS):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-fno-fast-math", "-fPIC", "-shared", SRC, "-o", OUT + f".{os.getpid()}.tmp"], check=True)
        os.replace(OUT + f".{os.getpid()}.tmp", OUT)
    L = ctypes.CDLL(OUT)
    L.posuv_map_many.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
    return L


def _map(L, rec, pos):
    rec = np.ascontiguousarray(rec)
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 4)
    out = np.empty((len(pos), 2), np.float32)
    L.posuv_map_many(rec.ctypes.data, pos.ctypes.data, len(pos), out.ctypes.data)
    return out


@pytest.mark.parametrize("name", pk.SCENES)
def test_mapping_equals_reference_on_recorded_hits(lib, name):
    a, maps = pk.uv_answers(name), pk.scene_index()[name]["mappings"]
    assert maps and (a["map"] >= 0).sum() >= 80
    for k, m in enumerate(maps):
        sel = a["map"] == k
        assert sel.any() and (a["position"][sel, 3] == 1).all()
        got = _map(lib, pk.mapping_record(m), a["position"][sel])
        bad = pk.same_bits(got, a["uv"][sel]).any(1)
        assert not bad.any(), (f"{name} mapping {k}: {int(bad.sum())} of {int(sel.sum())} differ, first position "
                               f"{a['position'][sel][bad][0]} got {got[bad][0]} want {a['uv'][sel][bad][0]}")


def test_fixture_mappings_cover_both_lengths():
    lens = {(len(m["origin"]), len(m["u_axis"]), len(m["v_axis"])) for n in pk.SCENES for m in pk.scene_index()[n]["mappings"]}
    assert {(3, 3, 3), (4, 3, 3), (4, 3, 4), (4, 4, 3)} <= lens


def _model(rec, pos):
    """materials.js:189-190 with Vec = Float32Array: numpy float64 arithmetic has no fused multiply-add."""
    o, p = rec["origin"].astype(np.float64), np.asarray(pos, np.float32).astype(np.float64)
    p = np.concatenate([p[:, :3], np.ones((len(p), 1))], 1)
    n = int(rec["origin_len"])
    with np.errstate(all="ignore"):
        delta = (o[None, :n] - p[:, :n]).astype(np.float32).astype(np.float64)
        out = []
        for ax, ln in (("u_axis", "u_len"), ("v_axis", "v_len")):
            a = rec[ax].astype(np.float64)
            s = a[0] * delta[:, 0] + a[1] * delta[:, 1]
            s = s + a[2] * delta[:, 2]
            if int(rec[ln]) == 4:
                s = s + a[3] * delta[:, 3]
            out.append(s.astype(np.float32))
    return np.stack(out, 1)


def test_constructed_cases(lib):
    e = np.float32(2.0 ** -24)
    inf = np.float32(np.inf)
    cases = []
    # (origin, u_axis, v_axis, positions)
    # 1 + 2^-24 + 2^-24: exact in f64 (1 + 2^-23), but f32 accumulation stops at 1 (two ties to even)
    cases.append(([1, e, e], [1, 1, 1], [1, 1, 0], [[0, 0, 0], [-0.0, -0.0, -0.0]]))
    # a tie of the single final rounding: 1 + 2^-24 -> 1 (even), 1 + 3 * 2^-24 -> 1 + 2^-22 (even)
    cases.append(([1, e, 0], [1, 1, 0], [1, 3, 0], [[0, 0, 0]]))
    # delta is rounded to f32 before the dot: 1 - 2^-25 is not an f32 (-> 1), so u = 3, not 3 - 3 * 2^-25 rounded
    cases.append(([1, 0, 0], [3, 0, 0], [0, 0, 0], [[2.0 ** -25, 0, 0], [-(2.0 ** -25), 0, 0]]))
    # signed zeros: delta +0 / -0, axes +-0; (+0) + (-0) = +0
    cases.append(([0.0, -0.0, 0.0], [-0.0, 0.0, -1.0], [1.0, -1.0, 0.0], [[0.0, 0.0, 0.0], [-0.0, 0.0, -0.0], [0.0, -0.0, 0.0]]))
    # infinities: inf - inf and 0 * inf are NaN, as in the reference
    cases.append(([inf, 1, -inf], [1, 0, 0], [0, 0, 1], [[0, 0, 0], [inf, 0, 0], [0, 0, -inf], [-inf, 5, inf]]))
    cases.append(([1, 2, 3], [0, inf, 0], [0, -inf, 1], [[0, 2, 0], [0, 1, 0], [0, 3, 0]]))
    # a 4-component origin with w != 1 under a 4-component axis (delta[3] = w - 1), and under a 3-component one
    cases.append(([1, 2, 3, 1.5], [1, 0, 0, 4], [0, 1, 0], [[0.25, 0.5, 0.75], [1, 2, 3]]))
    cases.append(([1, 2, 3, 1], [0.5, 0.25, 0.125, 1e30], [1, 1, 1, -1e30], [[0.25, 0.5, 0.75]]))
    cases.append(([1, 2, 3, 1 + 2.0 ** -23], [0, 0, 0, 2.0 ** 23], [1e-3, 0, 0, 1], [[1, 2, 3], [0.1, 0.2, 0.3]]))
    # magnitudes: products that need all 48 bits of the f64 product
    cases.append(([1.1, -2.3, 3.7], [0.3, 0.7, -0.9], [1e10, -1e10, 1e-10], [[0.1, 0.2, 0.3], [1e5, -1e5, 3.3], [1e-20, 0, 0]]))
    seen_nan = seen_neg0 = False
    for origin, ua, va, pos in cases:
        rec = pk.mapping_record({"origin": origin, "u_axis": ua, "v_axis": va})
        pos = np.concatenate([np.asarray(pos, np.float32), np.ones((len(pos), 1), np.float32)], 1)
        got, want = _map(lib, rec, pos), _model(rec, pos)
        bad = pk.same_bits(got, want)
        assert not bad.any(), f"origin {origin} axes {ua} {va}: got {got} want {want}"
        seen_nan |= bool(np.isnan(got).any())
        seen_neg0 |= bool(((got == 0) & np.signbit(got)).any())
    assert seen_nan and seen_neg0
    # the first case really separates the models
    rec = pk.mapping_record({"origin": [1, e, e], "u_axis": [1, 1, 1], "v_axis": [1, 1, 0]})
    got = _map(lib, rec, [[0, 0, 0, 1]])[0]
    assert got[0] == np.float32(1 + 2.0 ** -23) and got[1] == np.float32(1)
