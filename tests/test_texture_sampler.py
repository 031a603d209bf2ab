"""The texture sampler (jsraytracer_amd/csrc/texture_sample.h tex_sample), compiled for the host, against the
reference's own TextureMaterialColor.color (materials.js:101-130): every known answer of tests/golden/texture/
(tools/make_texture_fixtures.js: both modes, the four clamp combinations, sizes 1x1 .. 64x64; UVs at texel centres
and edges, 0, 1, -0, an f32 ulp either side of each, +-1e30, +-Infinity, NaN) bit for bit -- NaN where the
reference returns NaN, the same f32 everywhere else.  The chains over those textures (Scaled by a number, by a
Vec, a Checkerboard of two) are composed here from the sampler's output with mc_eval's arithmetic
(device_common.h), so that every case of the file is required on the CPU too."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import texture_kats as tk

ROOT = tk.ROOT
SRC = os.path.join(ROOT, "tests", "native", "texture_sample_host.hip")
OUT = os.path.join(ROOT, "tests", "native", "_build", "libtexture_sample_host.so")
HDRS = [os.path.join(ROOT, "jsraytracer_amd", "csrc", h) for h in ("texture_sample.h", "device_common.h")]
MODES = {"bilinear": 0, "nearest": 1}


@pytest.fixture(scope="module")
def lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(f) for f in [SRC] + HDRS):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-fno-fast-math", "-fPIC", "-shared", SRC, "-o", OUT + f".{os.getpid()}.tmp"], check=True)
        os.replace(OUT + f".{os.getpid()}.tmp", OUT)
    L = ctypes.CDLL(OUT)
    L.tex_sample_many.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
    return L


def _sample(L, case, uv):
    """The host sampler on the texture of a `texture` case (its descriptor and texels read from kats.jsrt)."""
    b = tk.blob("kats")
    rec = tk.records(b, "MCOL", tk.MCOL_DTYPE)[case["mcolor"]]
    assert rec["kind"] == tk.MC_TEXTURE
    t, img = tk.textures(b)[int(rec["a"])]
    assert [int(t["width"]), int(t["height"])] == case["size"] and int(t["mode"]) == MODES[case["mode"]]
    assert (bool(t["clamp_u"]), bool(t["clamp_v"])) == (case["clampU"], case["clampV"])
    desc = np.array([t["width"], t["height"], t["mode"], t["clamp_u"], t["clamp_v"]], np.uint32)
    texels = np.ascontiguousarray(img).copy()
    uv = np.ascontiguousarray(uv, np.float32)
    out = np.empty((len(uv), 3), np.float32)
    L.tex_sample_many(desc.ctypes.data, texels.ctypes.data, uv.ctypes.data, len(uv), out.ctypes.data)
    return out


CASES = tk.kats()
BY_ID = {c["id"]: c for c in CASES}


def _require(got, c):
    bad = tk.same_bits(got, c["want"]).any(1)
    assert not bad.any(), (f"{c['id']}: {int(bad.sum())} of {len(bad)} differ, first uv {c['uv'][bad][0]} "
                           f"got {got[bad][0]} want {c['want'][bad][0]}")


def test_fixture_covers_the_sweep():
    tex = [c for c in CASES if c["kind"] == "texture" and "_on_" not in c["id"]]
    assert len(tex) == 2 * 4 * 6 and {tuple(c["size"]) for c in tex} == {(1, 1), (1, 4), (4, 1), (2, 2), (5, 3), (64, 64)}
    assert {c["kind"] for c in CASES} == {"texture", "scaled_scalar", "scaled_vec", "checker"}
    for c in tex:
        u, v = c["uv"][:, 0], c["uv"][:, 1]
        assert np.isnan(u).any() and np.isnan(v).any() and (np.isnan(u) & np.isnan(v)).any()
        assert np.isinf(u).any() and np.isinf(v).any() and (np.abs(u) == np.float32(1e30)).any()
        assert ((u == 0) & np.signbit(u)).any() and ((u == 0) & ~np.signbit(u)).any() and (u == 1).any()
        assert np.isnan(c["want"]).any() and not np.isnan(c["want"]).all()
        assert len(c["uv"]) >= 600


@pytest.mark.parametrize("cid", [c["id"] for c in CASES if c["kind"] == "texture"])
def test_sampler_equals_reference(lib, cid):
    c = BY_ID[cid]
    _require(_sample(lib, c, c["uv"]), c)


def test_chains_over_textures_equal_reference(lib):
    """ScaledMaterialColor.color = child.color(data).times(scale) (f32 x f64 scalar in f64, rounded once; f32 x f32
    for a Vec scale), CheckerboardMaterialColor picks by floor(u) + floor(v) (materials.js:52-53, 72-75)."""
    c = BY_ID["scaled_scalar_5x3"]
    _require((_sample(lib, BY_ID[c["of"]], c["uv"]).astype(np.float64) * c["scale"]).astype(np.float32), c)
    c = BY_ID["scaled_vec_64x64"]
    _require(_sample(lib, BY_ID[c["of"]], c["uv"]) * np.array(c["scale"], np.float32), c)
    c = BY_ID["checker_5x3_2x2"]
    a = _sample(lib, BY_ID[c["a"]], c["uv"])
    b = (_sample(lib, BY_ID[c["b"]], c["uv"]).astype(np.float64) * c["b_scale"]).astype(np.float32)
    with np.errstate(invalid="ignore"):
        s = np.floor(c["uv"][:, 0].astype(np.float64)) + np.floor(c["uv"][:, 1].astype(np.float64))
        first = (s - np.floor(s / 2) * 2) < 1  # Math.fmod(s, 2) % 2 < 1; NaN / inf: false, the second colour
    _require(np.where(first[:, None], a, b), c)
    assert first.any() and (~first).any()
