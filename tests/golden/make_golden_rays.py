#!/usr/bin/env python3
"""Generate tests/golden/golden_rays.npz from the REFERENCE ITSELF: rays of the scattered
batches of tests/ray_batches.py (no camera generates them) with what the reference's public
bvh->intersect(Ray(o, d), hit_data) answers for each.

Runs only where oracle/_ref/ref_harness exists (compiled from the unmodified reference sources
by `make -C oracle ref`): its `anyrays` command reads 24-B (o, d) records and writes the 32-B
record {d, t, normal, hit} of its `rays` command.  Per scene, RAYS rays drawn (seeded) from the
`mixed` batch, so every family is represented; stored are their indices in that batch, the rays
and the records (d is checked to pass through untouched and not stored twice).  Data only.

usage: python tests/golden/make_golden_rays.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import ray_batches  # noqa: E402
import rq_util  # noqa: E402

HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
SCENES = ["soup1", "hf_small", "single_sphere"]
RAYS = 2048


def sample(n):
    """The seeded indices of the stored rays within a `mixed` batch of n rays."""
    return np.sort(np.random.default_rng(800).choice(n, RAYS, replace=False)).astype(np.int32)


def reference_records(xml, o, d):
    with tempfile.TemporaryDirectory() as tmp:
        rays, out = os.path.join(tmp, "rays.bin"), os.path.join(tmp, "out.bin")
        np.concatenate([o, d], axis=1).astype(np.float32).tofile(rays)
        subprocess.run([HARNESS, "anyrays", xml, rays, out], check=True, stdout=subprocess.DEVNULL)
        return np.fromfile(out, np.float32).reshape(-1, 8)


def main():
    if not os.path.exists(HARNESS):
        sys.exit("reference harness missing: run `make -C oracle ref` first")
    arrays = {}
    with tempfile.TemporaryDirectory() as d:
        for name in SCENES:
            xml = rq_util.scene_xml(name, d)
            b = ray_batches.family(ray_batches.scene_info(xml, name), "mixed")
            idx = sample(len(b))
            o, dd = b.o[idx], b.d[idx]
            rec = reference_records(xml, o, dd)
            assert len(rec) == RAYS
            assert np.array_equal(rec[:, 0:3].view(np.uint32), dd.view(np.uint32))
            hit = rec[:, 7] == 1.0
            arrays[name + "__index"] = idx
            arrays[name + "__part"] = b.part[idx]
            arrays[name + "__o"] = o
            arrays[name + "__d"] = dd
            arrays[name + "__t"] = rec[:, 3].copy()
            arrays[name + "__normal"] = rec[:, 4:7].copy()
            arrays[name + "__hit"] = hit.astype(np.uint8)
            print(name, len(b), "rays in the batch;", int(hit.sum()), "of", RAYS, "stored hit;",
                  "parts", np.bincount(b.part[idx]).tolist(), flush=True)
    path = os.path.join(HERE, "golden_rays.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
