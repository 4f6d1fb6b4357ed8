#!/usr/bin/env python3
"""Generate tests/golden/golden_hw3.npz and golden_hw3.json from the REFERENCE ITSELF: the
unmodified HW3 sources behind oracle/_ref/hw3_harness (`make -C oracle ref-hw3`), put the scenes
and rays of tests/ref34_util.py (HW3_CASES: smooth shading with and without a tiny area light,
glass with the present Transparency and with 1 1 1, mesh instances, motion blur).

Per scene: the rays (o, d, time), the `hits` records (hit, t, normal, material), Scene::trace_ray
of every ray outside and inside a medium, the loader's vertex normals, and per ray the departure
classes of its restated tree; the .json holds the SHA-256 of every scene file and the counts.
Every harness command runs twice and must give the same bytes.  Data only.

usage: python tests/golden/make_golden_hw3.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref34_util  # noqa: E402

if __name__ == "__main__":
    ref34_util.write_golden(3)
