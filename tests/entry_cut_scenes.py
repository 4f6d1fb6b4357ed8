"""Scenes of the entry-cut tests: small scenes whose cameras meet the cases the
host builder decides — a tree of several levels, ragged tiles, a camera inside the root box and
one far away, directions with zero components, two cameras, and scenes moved and resized."""
from __future__ import annotations

import os

import scenes
from scenes import G


def _hf():
    # 25 x 17 tiles over the 48 x 48 height field seen from above
    return G.heightfield_scene(48, 200, 136)


def _inside():
    spec = G.soup_scene(2, 64, 48)
    pts = [[float(t) for t in ln.split()] for ln in spec.vertex_text.split("\n")]
    lo = [min(p[a] for p in pts) for a in range(3)]
    hi = [max(p[a] for p in pts) for a in range(3)]
    mid = tuple(0.5 * (l + h) for l, h in zip(lo, hi))
    spec.cameras = [G.Camera(mid, (0.3, -0.2, -1), (0, 1, 0), (-1, 1, -0.75, 0.75), 1, 64, 48,
                             "inside.png")]
    return spec


def _far():
    # the field's box has a diagonal of about 8.5: the camera hangs 100 diagonals above it
    spec = G.heightfield_scene(48, 64, 64)
    spec.cameras = [G.Camera((0, 850.0, -5), (0, -1, 0), (0, 0, -1),
                             (-0.004, 0.004, -0.004, 0.004), 1, 64, 64, "far.png")]
    return spec


def _axis():
    # gaze along -z, odd sides: the centre column has d_x = 0 and the centre row d_y = 0
    spec = G.heightfield_scene(48, 65, 49)
    spec.cameras = [G.Camera((0, 0.5, 1.0), (0, 0, -1), (0, 1, 0), (-1, 1, -1, 1), 1, 65, 49,
                             "axis.png")]
    return spec


def _two_cameras():
    return G.heightfield_scene(32, 64, 48, cameras=2)


# name -> (factory, cameras)
SCENES = {
    "cut_hf": (_hf, 1),
    "cut_ragged": (scenes.SPLIT["ragged"][0], None),
    "cut_inside": (_inside, 1),
    "cut_far": (_far, 1),
    "cut_axis": (_axis, 1),
    "cut_two": (_two_cameras, 2),
    "cut_s2m20": (scenes.PLACED["hf@s2m20"][0], 1),
    "cut_t1e5": (scenes.PLACED["soup@t1e5"][0], None),
}


def write(name: str, directory: str) -> str:
    path = os.path.join(directory, f"{name}.xml")
    if not os.path.exists(path):
        tmp = path + ".tmp"
        with open(tmp, "w") as f:
            f.write(SCENES[name][0]().to_xml())
        os.replace(tmp, path)
    return path
