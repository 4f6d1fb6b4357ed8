#!/usr/bin/env python3
"""Generate tests/golden/golden_hw4.npz and golden_hw4.json from the REFERENCE ITSELF: the
unmodified HW4 sources behind oracle/_ref/hw4_harness (`make -C oracle ref-hw4`), put
texture_util.textured_xml's scene without the loose triangle's <Texture> (HW4 leaves that
triangle's u, v unwritten), with the present glass and with Transparency 1 1 1, images as binary
PPM files under the names the scene gives them.

Per scene: the rays, the `hits` records (hit, t, normal, material, u, v, texture),
Scene::trace_ray of every ray outside and inside a medium, the vertex normals, the departure
classes, and Texture::get_color_at at the uv of every textured hit.  `texels`: get_color_at on
texture_util.grid_queries for every size of SIZES in every mode of MODES.  Queries whose index
arithmetic (HW4/src/Texture.cpp:108-111, under the guards of :115-129) reaches 3 w h are dropped
by that formula and counted in the .json.  Every harness command runs twice and must give the
same bytes.  Data only.

usage: python tests/golden/make_golden_hw4.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref34_util  # noqa: E402

if __name__ == "__main__":
    ref34_util.write_golden(4)
