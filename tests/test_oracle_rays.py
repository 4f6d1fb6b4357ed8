"""Pin the oracle's per-ray entries (OracleScene.intersect_rays / shade_rays) and the scattered
ray batches of tests/ray_batches.py.  CPU only.

intersect_rays and shade_rays add no arithmetic: they run the oracle's Scene::intersect and
Scene::trace on a caller's Ray{o, d, in_medium}.  Three pins:
  * camera rays: intersect_rays(camera position, primary_records' d) is primary_records, and
    shade_rays(depth=-1) is render(cam), bit for bit with equal ray counts;
  * the reference itself: tests/golden/golden_rays.npz holds rays of the scattered batches with
    the answers of the reference's public bvh->intersect (make_golden_rays.py through
    ref_harness `anyrays`); the generator must still produce those rays byte for byte, and the
    oracle those answers;
  * radiance has no pin beyond the camera one: Scene::trace_ray is private in the reference, so
    no harness command can call it with a caller's ray.  What shade_rays adds to trace — the
    loop, the `in_medium` member and the depth argument — are plain arguments of a function the
    frames already pin.
Then every family's mix conditions on every scene the GPU tests use it with, from the oracle
alone."""
import os

import numpy as np
import pytest

import ray_batches as rb
import rq_util
import scenes
from oracle.cpu_ref import OracleScene

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "golden_rays.npz"))
PIN_SCENES = ["soup1", "single_sphere", "hf_small", "soup_depth3"]
BATCH_SCENES = ["soup1", "hf_small", "single_sphere", "deep", "soup_depth3", "soup_depth6"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", PIN_SCENES)
def test_intersect_rays_is_primary_records(scene_dir, name):
    xml = scenes.write(name, scene_dir)
    o = OracleScene(xml)
    pos = rq_util.camera_positions(xml)
    assert o.num_cameras == len(pos) >= 1
    for cam in range(o.num_cameras):
        want = o.primary_records(cam).reshape(-1, 8)
        got, shape = o.intersect_rays(np.broadcast_to(pos[cam], (len(want), 3)), want[:, 0:3])
        assert np.array_equal(bits(got), bits(want)), (name, cam)
        assert np.array_equal(shape >= 0, want[:, 7] == 1.0)
        assert (want[:, 7] == 1.0).sum() >= 100


@pytest.mark.parametrize("name", PIN_SCENES)
def test_shade_rays_is_render(scene_dir, name):
    xml = scenes.write(name, scene_dir)
    o = OracleScene(xml)
    pos = rq_util.camera_positions(xml)
    for cam in range(o.num_cameras):
        frame, fst = o.render(cam, threads=4)
        rec = o.primary_records(cam).reshape(-1, 8)
        got, st = o.shade_rays(np.broadcast_to(pos[cam], (len(rec), 3)), rec[:, 0:3], depth=-1,
                               in_medium=False)
        assert np.array_equal(bits(got[:, 0:3]), bits(frame.reshape(-1, 3))), (name, cam)
        hit = rec[:, 7] == 1.0
        assert np.array_equal(bits(got[hit, 3]), bits(rec[hit, 3]))
        assert (bits(got[~hit, 3]) == bits(np.float32(np.inf))).all()
        assert fst.as_dict() == st.as_dict(), (name, cam)
    if name == "soup_depth3":
        assert st.secondary_rays >= 100 and st.shadow_rays >= 100


@pytest.mark.parametrize("name", ["soup1", "hf_small", "single_sphere"])
def test_golden_rays(scene_dir, name):
    """The stored rays are still what the generator makes (else the fixture pins other rays than
    the GPU tests trace), and the oracle gives the reference's answer for each."""
    xml = rq_util.scene_xml(name, scene_dir)
    b = rb.family(rb.scene_info(xml, name), "mixed")
    idx = GOLDEN[name + "__index"]
    assert len(idx) <= 2048 and len(np.unique(GOLDEN[name + "__part"])) == len(rb.PARTS)
    assert b.o[idx].tobytes() == GOLDEN[name + "__o"].tobytes()
    assert b.d[idx].tobytes() == GOLDEN[name + "__d"].tobytes()
    assert np.array_equal(b.part[idx], GOLDEN[name + "__part"])
    o = OracleScene(xml)
    rec, _ = o.intersect_rays(GOLDEN[name + "__o"], GOLDEN[name + "__d"])
    o.close()
    assert np.array_equal(bits(rec[:, 0:3]), bits(GOLDEN[name + "__d"]))  # d passes through
    assert np.array_equal(rec[:, 7] == 1.0, GOLDEN[name + "__hit"] == 1)
    assert np.array_equal(bits(rec[:, 3]), bits(GOLDEN[name + "__t"]))
    assert np.array_equal(bits(rec[:, 4:7]), bits(GOLDEN[name + "__normal"]))
    assert 100 <= int(GOLDEN[name + "__hit"].sum()) <= len(idx) - 100 or name == "single_sphere"


def test_golden_rays_file_is_small():
    here = os.path.join(HERE, "golden")
    assert os.path.getsize(os.path.join(here, "golden_rays.npz")) <= \
        os.path.getsize(os.path.join(here, "golden.npz"))


@pytest.mark.parametrize("family", rb.FAMILIES)
@pytest.mark.parametrize("name", BATCH_SCENES)
def test_mix_conditions(scene_dir, name, family):
    xml = rq_util.scene_xml(name, scene_dir)
    info = rb.scene_info(xml, name)
    b = rb.family(info, family)
    assert b.o.dtype == b.d.dtype == np.float32 and len(b) <= 8192
    o = OracleScene(xml)
    rec, shape = o.intersect_rays(b.o, b.d)
    o.close()
    got = rb.check_mix(info, b, rec, shape)
    print(name, family, got)
    # inside what DESIGN.md §4.11 claims: finite, |o_a| <= 2^100, not all |d_a| < 1e-6
    assert np.isfinite(b.o).all() and np.isfinite(b.d).all()
    assert (np.abs(b.o) <= np.float32(2.0 ** 100)).all()
    assert not (np.abs(b.d) < rb.EPS_SKIP).all(axis=1).any()
    # the same bytes when made again
    again = rb.family(info, family)
    assert again.o.tobytes() == b.o.tobytes() and again.d.tobytes() == b.d.tobytes()


@pytest.mark.parametrize("name", BATCH_SCENES)
def test_mixed_batch(scene_dir, name):
    xml = rq_util.scene_xml(name, scene_dir)
    b = rb.family(rb.scene_info(xml, name), "mixed")
    assert len(b) < 40000 and len(np.unique(b.part)) == len(rb.PARTS)
    perm = rb.permutation(b)
    assert np.array_equal(np.sort(perm), np.arange(len(b)))
    own = b.part == rb.PARTS["surface_c"]
    assert np.isnan(b.tmax[~own]).all() and (b.tmax[own] > 0).all()


@pytest.mark.parametrize("name", ["soup_depth3", "soup_depth6"])
def test_in_medium_and_depth_change_colours(scene_dir, name):
    """The radiance grid is not vacuous: on the dielectric scenes in_medium changes at least 100
    colours at every depth above 0, and the depth argument changes at least 100."""
    xml = rq_util.scene_xml(name, scene_dir)
    b = rb.family(rb.scene_info(xml, name), "surface")
    o = OracleScene(xml)
    rad = {(k, m): o.shade_rays(b.o, b.d, depth=k, in_medium=m)[0] for k in (0, 1, -1)
           for m in (False, True)}

    def changed(x, y):
        return int((bits(x[:, 0:3]) != bits(y[:, 0:3])).any(axis=1).sum())
    for k in (0, 1, -1):
        assert changed(rad[k, False], rad[k, True]) >= 100, k
        assert np.array_equal(bits(rad[k, False][:, 3]), bits(rad[k, True][:, 3]))
    assert changed(rad[0, False], rad[1, False]) >= 100
    assert changed(rad[1, False], rad[-1, False]) >= 100
    with pytest.raises(RuntimeError):
        o.shade_rays(b.o[:4], b.d[:4], depth=99)
