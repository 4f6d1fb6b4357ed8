"""Scenes moved and resized: placed(spec, scale, offset) maps a SceneSpec through
p -> scale * p + offset so that every camera sees the picture it saw before, up to rounding.

What is transformed: vertices, camera positions and light positions as points; sphere radii, the
near plane's four bounds, the near distance and the shadow-ray epsilon as lengths (x scale);
light intensities x scale^2 (the reference divides them by the squared distance,
HW2/Scene.cpp:124-126).  Gaze and up vectors, materials, colours and the recursion depth stay.

Every number is first taken as the fp32 value the loaders read from the base scene's text, mapped
in double, rounded to fp32 and written as %.9g of that value (SceneSpec.number_format): nine
digits name an fp32 value uniquely, where gen_scene's %.6f would erase a scene of size 2^-30.
With a power-of-two scale and no offset the map is exact, so a scene of triangles renders the
base frame bit for bit (tests/test_placed_host.py holds the height field to that)."""
from __future__ import annotations

import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_scene as G  # noqa: E402

NUMBER_FORMAT = "%.9g"


def f32(x) -> float:
    return float(np.float32(x))


def placed(spec: G.SceneSpec, scale: float, offset=(0.0, 0.0, 0.0)) -> G.SceneSpec:
    s = float(scale)
    T = tuple(float(t) for t in offset)

    def length(x):
        return f32(f32(x) * s)

    def point(p):
        return tuple(f32(f32(c) * s + t) for c, t in zip(p, T))

    out = copy.deepcopy(spec)
    out.number_format = NUMBER_FORMAT
    lines = []
    for ln in spec.vertex_text.split("\n"):
        x, y, z = point(float(tok) for tok in ln.split())
        lines.append(f"{NUMBER_FORMAT} {NUMBER_FORMAT} {NUMBER_FORMAT}" % (x, y, z))
    out.vertex_text = "\n".join(lines)
    for c in out.cameras:
        c.position = point(c.position)
        c.near_plane = tuple(length(v) for v in c.near_plane)
        c.near_distance = length(c.near_distance)
    out.lights = [(point(p), tuple(f32(f32(i) * s * s) for i in inten))
                  for p, inten in spec.lights]
    out.spheres = [(m, c, length(r)) for m, c, r in spec.spheres]
    if spec.shadow_eps is not None:
        out.shadow_eps = length(spec.shadow_eps)
    return out
