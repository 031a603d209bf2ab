"""Readers of tests/golden/posuv/ (written by tools/make_posuv_fixtures.js from the reference itself), shared by the
PositionalUVMaterial tests: the five thumbnail scenes, their reference renders, the per-hit UV answers, and a small
JSRT blob editor (include/jsrt_scene.h) for the shapes the loader must refuse."""
import base64
import functools
import gzip
import json
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "golden", "posuv")
SCENES = ("flat", "flat_plain", "box", "mesh", "sdf")
MAT_POSITIONAL_UV = 6  # JSRT_MAT_POSITIONAL_UV
MC_TEXTURE = 5         # JSRT_MC_TEXTURE
MATL_DTYPE = np.dtype([("kind", "<u4"), ("base", "<i4"), ("ambient", "<i4"), ("diffuse", "<i4"), ("specular", "<i4"),
                       ("reflect", "<i4"), ("transmit", "<i4"), ("color", "<i4"), ("smoothness", "<f8"), ("ratio", "<f8"),
                       ("mirror_prob", "<f8"), ("opacity", "<f8")])
PUVM_DTYPE = np.dtype([("origin", "<f4", 4), ("u_axis", "<f4", 4), ("v_axis", "<f4", 4), ("origin_len", "<u4"),
                       ("u_len", "<u4"), ("v_len", "<u4"), ("pad", "<u4")])
MCOL_DTYPE = np.dtype([("kind", "<u4"), ("a", "<i4"), ("b", "<i4"), ("len", "<u4"), ("vec", "<f4", 4), ("scalar", "<f8")])
OBJS_DTYPE = np.dtype([("kind", "<u4"), ("geometry", "<i4"), ("material", "<i4"), ("casts_shadow", "<u4"),
                       ("first_child", "<i4"), ("n_children", "<i4"), ("bvh_root", "<i4"), ("matrix", "<i4")])
assert MATL_DTYPE.itemsize == 64 and PUVM_DTYPE.itemsize == 64 and OBJS_DTYPE.itemsize == 32


def _gz(name):
    with gzip.open(os.path.join(DIR, name + ".gz"), "rb") as f:
        return f.read()


@functools.lru_cache(None)
def blob(name):
    return _gz(name + ".jsrt")


def serializer_json(name):
    return _gz(name + ".json")


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


@functools.lru_cache(None)
def uv_answers(name):
    """rays (n x 6), uv (n x 2, NaN = none), has_uv (n), position (n x 4), map (n: index into mappings, -1 none)."""
    d = json.loads(_gz(name + ".uv.json"))
    arr = lambda k, t: np.frombuffer(base64.b64decode(d[k]), t)
    return {"n": d["n"], "n_primary": d["n_primary"], "rays": arr("rays", np.float32).reshape(-1, 6),
            "uv": arr("uv", np.float32).reshape(-1, 2), "has_uv": arr("has_uv", np.int32),
            "position": arr("position", np.float32).reshape(-1, 4), "map": arr("map", np.int32)}


def mapping_record(m):
    """A scenes.json mapping ({origin, u_axis, v_axis}: the wrapper's Vecs) as a PUVM record."""
    r = np.zeros((), PUVM_DTYPE)
    for k, n in (("origin", "origin_len"), ("u_axis", "u_len"), ("v_axis", "v_len")):
        r[k][:len(m[k])] = m[k]
        r[n] = len(m[k])
    return r


def same_bits(got, want):
    """The mask of f32 elements that differ bit for bit (any NaN equals any NaN)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))


def sections(b):
    """[(tag, count, payload bytes)] of a JSRT blob, in file order."""
    magic, version, nsec, _ = struct.unpack_from("<4I", b, 0)
    assert magic == 0x5452534A and version == 1
    out = []
    for i in range(nsec):
        tag, count, off, nbytes = struct.unpack_from("<IIQQ", b, 16 + 24 * i)
        out.append((struct.pack("<I", tag).decode(), count, bytes(b[off:off + nbytes])))
    return out


def records(b, tag, dtype):
    for t, count, payload in sections(b):
        if t == tag:
            return np.frombuffer(payload, dtype, count).copy()
    return np.zeros(0, dtype)


def rebuild(b, **replace):
    """The blob with the records of the named sections replaced (TAG=numpy record array), laid out as
    scene_blob.js serialize() does: header, descriptors, payloads 8-byte aligned, in the same order."""
    secs = []
    for tag, count, payload in sections(b):
        if tag in replace:
            a = np.ascontiguousarray(replace[tag])
            count, payload = len(a), a.tobytes()
        secs.append((tag, count, payload))
    off = (16 + 24 * len(secs) + 7) & ~7
    head = [struct.pack("<4I", 0x5452534A, 1, len(secs), 0)]
    body = b""
    for tag, count, payload in secs:
        head.append(struct.pack("<4sIQQ", tag.encode(), count, off + len(body), len(payload)))
        body += payload + b"\0" * (-len(payload) % 8)
    h = b"".join(head)
    return h + b"\0" * (off - len(h)) + body
