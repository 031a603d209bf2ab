"""Readers of tests/golden/mtlmap/ (written by tools/make_posuv_fixtures.js from the reference itself): an OBJ and
MTL of this project's own with map_Ka / map_Kd / map_Ks, built by the reference's loadObjFile / parseMtlFile with the
seeded images, exported (full.jsrt) and rendered (simple, incremental); skel.jsrt is the input of the native ingest."""
import functools
import gzip
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "golden", "mtlmap")
RENDERS = ("simple", "incremental")


def _gz(name):
    with gzip.open(os.path.join(DIR, name + ".gz"), "rb") as f:
        return f.read()


@functools.lru_cache(None)
def index():
    with open(os.path.join(DIR, "scenes.json")) as f:
        return json.load(f)


@functools.lru_cache(None)
def blob(name):  # "skel" / "full"
    return _gz(name + ".jsrt")


def text(name):  # "scene.obj" / "scene.mtl"
    with open(os.path.join(DIR, name)) as f:
        return f.read()


def textures():
    """{file name: H x W x 4 uint8}"""
    return {k: np.frombuffer(_gz(v["file"]), np.uint8).reshape(v["height"], v["width"], 4)
            for k, v in index()["textures"].items()}


def golden_image(name):
    r = index()["renders"][name]
    W, H = r["width"], r["height"]
    return (np.frombuffer(_gz(name + ".f32"), np.float32).reshape(H, W, 4),
            np.frombuffer(_gz(name + ".rgba"), np.uint8).reshape(H, W, 4))
