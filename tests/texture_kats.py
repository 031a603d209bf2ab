"""Readers of tests/golden/texture/ (written by tools/make_texture_fixtures.js from the reference itself), shared by
the texture tests: the known answers of TextureMaterialColor.color, the four thumbnail scenes and their reference
renders, and the texture records of a JSRT blob (include/jsrt_scene.h)."""
import functools
import gzip
import json
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "golden", "texture")
SCENES = ("flat", "box", "mesh", "cylinder")
MC_TEXTURE = 5  # JSRT_MC_TEXTURE
MCOL_DTYPE = np.dtype([("kind", "<u4"), ("a", "<i4"), ("b", "<i4"), ("len", "<u4"), ("vec", "<f4", 4), ("scalar", "<f8")])
TEXR_DTYPE = np.dtype([("width", "<u4"), ("height", "<u4"), ("mode", "<u4"), ("clamp_u", "<u4"), ("clamp_v", "<u4"),
                       ("pad", "<u4"), ("offset", "<u8")])


def _gz(name):
    with gzip.open(os.path.join(DIR, name + ".gz"), "rb") as f:
        return f.read()


@functools.lru_cache(None)
def blob(name):
    return _gz(name + ".jsrt")


def sections(b):
    """{tag: (count, offset, bytes)} of a JSRT blob."""
    magic, version, nsec, _ = struct.unpack_from("<4I", b, 0)
    assert magic == 0x5452534A and version == 1
    out = {}
    for i in range(nsec):
        tag, count, off, nbytes = struct.unpack_from("<IIQQ", b, 16 + 24 * i)
        out[struct.pack("<I", tag).decode()] = (count, off, nbytes)
    return out


def records(b, tag, dtype):
    count, off, nbytes = sections(b).get(tag, (0, 0, 0))
    assert nbytes == count * dtype.itemsize
    return np.frombuffer(b, dtype, count, off)


def textures(b):
    """[(descriptor record, (H, W, 4) uint8 image)] of a blob's TEXR / TEXL sections."""
    tex = records(b, "TEXR", TEXR_DTYPE)
    _, toff, tbytes = sections(b).get("TEXL", (0, 0, 0))
    out = []
    for t in tex:
        w, h, o = int(t["width"]), int(t["height"]), int(t["offset"])
        assert o + w * h * 4 <= tbytes
        out.append((t, np.frombuffer(b, np.uint8, w * h * 4, toff + o).reshape(h, w, 4)))
    return out


@functools.lru_cache(None)
def kats():
    """(cases, f32 array): every case with uv (n x 2) and want (n x 3) views added."""
    meta = json.loads(_gz("kats.json"))
    f = np.frombuffer(_gz("kats.bin"), np.float32)
    cases = []
    for c in meta["cases"]:
        s = meta["uv_sets"][c["uv_set"]]
        assert s["n"] == c["n"]
        c = dict(c, uv=f[s["offset"]:s["offset"] + 2 * s["n"]].reshape(-1, 2),
                 want=f[c["offset"]:c["offset"] + 3 * c["n"]].reshape(-1, 3))
        cases.append(c)
    return cases


def same_bits(got, want):
    """Bit-for-bit equality of f32 arrays, any NaN equal to any NaN (the reference's NaNs are canonical; a device
    NaN's payload is not part of the contract): the mask of elements that differ."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))


@functools.lru_cache(None)
def scene_index():
    with open(os.path.join(DIR, "scenes.json")) as f:
        return json.load(f)


def golden_image(name):
    r = scene_index()[name]
    W, H = r["width"], r["height"]
    rgba = np.frombuffer(_gz(name + ".rgba"), np.uint8).reshape(H, W, 4)
    col = np.frombuffer(_gz(name + ".f32"), np.float32).reshape(H, W, 4)
    return col, rgba
