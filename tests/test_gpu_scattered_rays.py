"""Ray and radiance queries on rays no camera can generate, against the CPU oracle's per-ray
entries (OracleScene.intersect_rays / shade_rays, pinned to the reference by
tests/test_oracle_rays.py), bit for bit.

The batches are the seeded families of tests/ray_batches.py — 64 different origins per wave,
inside the boxes, on surfaces with and without epsilon, shadow rays built as Scene.cpp builds
them, directions scaled over 72 binades, components at the slab test's 1e-6 threshold, origin
coordinates outside the shared-reciprocal range — each alone, under one seeded permutation,
and concatenated (`mixed`).  tests/test_oracle_rays.py asserts every family's mix conditions on
every scene used here, from the oracle alone, so no batch is vacuous; the cheap ones are
re-asserted here where the expected values are at hand."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import desc_xml
import ray_batches as rb
import rq_util
from conftest import assert_parity
from oracle.cpu_ref import OracleScene
from rq_util import INF, assert_hits_match, bits, occlusion, same_records, shade_device, trace

pytestmark = pytest.mark.gpu

SCENES = ["soup1", "hf_small", "single_sphere", "deep"]
FAMILIES = list(rb.FAMILIES) + ["mixed"]
MODES = ["fast", "reference"]
GLASS = ["soup_depth3", "soup_depth6"]


# ---------------------------------------------------------------- shared, computed once
@functools.lru_cache(maxsize=None)
def expected(xml, name, family):
    """(batch, the oracle's records as assert_hits_match reads them, its hit objects)."""
    b = rb.family(rb.scene_info(xml, name), family)
    o = OracleScene(xml)
    rec, shape = o.intersect_rays(b.o, b.d)
    o.close()
    nan_t = np.isnan(rec[:, 3])
    row = rec[nan_t]
    row[np.isnan(row)] = np.nan  # (see canonical_nans)
    rec[nan_t] = row
    for a in (b.o, b.d, rec, shape, nan_t):
        a.setflags(write=False)
    want = SimpleNamespace(hit=rec[:, 7] == 1.0, t=rec[:, 3], normal=rec[:, 4:7], shape=shape,
                           nan_t=nan_t)
    return b, want


@functools.lru_cache(maxsize=None)
def expected_radiance(xml, name, family, depth, in_medium):
    b = rb.family(rb.scene_info(xml, name), family)
    o = OracleScene(xml)
    rad, st = o.shade_rays(b.o, b.d, depth=depth, in_medium=in_medium)
    o.close()
    rad.setflags(write=False)
    return b, rad, st.as_dict()


@functools.lru_cache(maxsize=None)
def leaf_objects(xml):
    import ceng795_amd
    desc = desc_xml.Desc(xml)  # (owns the arrays its rt_scene_desc points at)
    return ceng795_amd.host_leaf_objects(desc.d)


@pytest.fixture(scope="module")
def gpu_scene():
    """One ceng795_amd.Scene per (xml, traversal), shared by the module's tests."""
    import ceng795_amd
    opened = {}

    def get(xml, traversal="fast"):
        if (xml, traversal) not in opened:
            opened[xml, traversal] = ceng795_amd.Scene(xml, traversal=traversal)
        return opened[xml, traversal]
    yield get
    for s in opened.values():
        s.close()


NAN_T = {("single_sphere", "range"): 818, ("single_sphere", "mixed"): 818}


def canonical_nans(hits, nan_t):
    """A copy of the hit records in which the rays whose oracle t is NaN (`nan_t`) have the NaNs
    of their t and normal replaced by the one quiet NaN 0x7fc00000; expected() does the same to
    the oracle's records of those rays.  A lone root sphere whose discriminant is inf - inf is a
    hit with t = NaN in the reference (Sphere.h:33-49: no comparison rejects a NaN); IEEE 754
    leaves the sign and payload of an invalid operation's NaN open, x86 SSE gives 0xffc00000 and
    the GPU 0x7fc00000.  So these rays — NAN_T: single_sphere's 818 `range` rays with a 2^49 or
    2^60 origin, and no ray of any other scene or family, which test_closest_hit asserts — are
    held to "NaN where the oracle has NaN", and every other ray to the oracle's bits."""
    hits = hits.copy()
    for f in ("t", "normal"):
        v = hits[f][nan_t]
        v[np.isnan(v)] = np.nan
        hits[f][nan_t] = v
    return hits


def report(what, hits, want):
    """Print, before any assertion, how many rays differ and the first one (read with -s)."""
    got_hit = hits["leaf"] >= 0
    both = got_hit & want.hit
    wrong = (got_hit != want.hit) | (both & (bits(hits["t"]) != bits(want.t))) | \
        (both & (bits(hits["normal"]) != bits(want.normal)).any(axis=1))
    print(f"{what}: {len(want.t)} rays, {int(want.hit.sum())} hits, {int(wrong.sum())} differ")
    return wrong


# ---------------------------------------------------------------- 1. closest hit
@pytest.mark.parametrize("reorder", [False, True])
@pytest.mark.parametrize("traversal", MODES)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", SCENES)
def test_closest_hit(scene_dir, gpu_scene, name, family, traversal, reorder):
    xml = rq_util.scene_xml(name, scene_dir)
    b, want = expected(xml, name, family)
    assert len(b) < 40000 and want.hit.any()
    s = gpu_scene(xml, traversal)
    raw, _ = trace(s, b.o, b.d, reorder=reorder)
    assert int(want.nan_t.sum()) == NAN_T.get((name, family), 0)
    hits = canonical_nans(raw, want.nan_t)
    what = f"{name}/{family}/{traversal}/reorder{reorder}"
    wrong = report(what, hits, want)
    if wrong.any():
        k = int(np.flatnonzero(wrong)[0])
        print(f"  first: ray {k} part {b.part[k]} o {b.o[k]} d {b.d[k]} got t {hits['t'][k]!r} "
              f"leaf {hits['leaf'][k]} want hit {want.hit[k]} t {want.t[k]!r}")
    assert_hits_match(hits, want, what)
    hit = want.hit
    assert np.array_equal(hits["object"][hit], leaf_objects(xml)[hits["leaf"][hit]]), what
    assert np.array_equal(hits["object"][hit], want.shape[hit]), what
    perm = rb.permutation(b)
    mixed, _ = trace(s, b.o[perm], b.d[perm], reorder=reorder)
    assert same_records(mixed, raw[perm]), what + "/permuted"


# ---------------------------------------------------------------- 2. occlusion
@pytest.mark.parametrize("reorder", [False, True])
@pytest.mark.parametrize("traversal", MODES)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", SCENES)
def test_occlusion(scene_dir, gpu_scene, name, family, traversal, reorder):
    """tmax = dist - eps on the shadow rays of surface(c), as Scene.cpp:124 compares; on every
    other ray the cycle {t, just above, just below, t/2, 2t, 0, -1, inf, NaN} of the oracle's t."""
    xml = rq_util.scene_xml(name, scene_dir)
    b, want = expected(xml, name, family)
    tmax = rb.occlusion_tmax(b, want.t)
    with np.errstate(invalid="ignore"):
        occ = (want.hit & (want.t > 0) & (want.t < tmax)).astype(np.uint8)
    if b.tmax is not None:
        own = b.part == rb.PARTS["surface_c"]
        assert (occ[own] == 1).sum() >= 300 and (occ[own] == 0).sum() >= 300
    assert occ.sum() >= 10 and (want.hit & (occ == 0)).sum() >= 10
    s = gpu_scene(xml, traversal)
    got, _ = occlusion(s, b.o, b.d, tmax, reorder=reorder)
    what = f"{name}/{family}/{traversal}/reorder{reorder}"
    print(f"{what}: {len(b)} rays, {int(occ.sum())} occluded, {int((got != occ).sum())} differ")
    assert np.array_equal(got, occ), what
    perm = rb.permutation(b)
    mixed, _ = occlusion(s, b.o[perm], b.d[perm], tmax[perm], reorder=reorder)
    assert np.array_equal(mixed, occ[perm]), what + "/permuted"


# ---------------------------------------------------------------- 3. radiance
def radiance_case(s, xml, name, depth, in_medium, what):
    b, want, counts = expected_radiance(xml, name, "mixed", depth, in_medium)
    rad, st = s.shade_rays(b.o, b.d, depth=None if depth < 0 else depth, in_medium=in_medium,
                           stats=True)
    differ = (bits(rad["rgb"]) != bits(want[:, 0:3])).any(axis=1)
    print(f"{what}: {len(b)} rays, {int(differ.sum())} colours and "
          f"{int((bits(rad['t']) != bits(want[:, 3])).sum())} t differ in bits; "
          f"{int(np.isnan(rad['rgb']).any(axis=1).sum())} NaN and "
          f"{int(np.isinf(rad['rgb']).any(axis=1).sum())} infinite colours, "
          f"{st.shadow_rays} shadow and {st.secondary_rays} secondary rays")
    nbad = assert_parity(rad["rgb"], np.ascontiguousarray(want[:, 0:3]), what)
    assert np.array_equal(bits(rad["t"]), bits(want[:, 3])), what
    for k in ("primary_rays", "shadow_rays", "secondary_rays"):
        assert getattr(st, k) == counts[k], (what, k, getattr(st, k), counts[k])
    return b, rad, want, nbad


@pytest.mark.parametrize("traversal", MODES)
def test_radiance_flat(scene_dir, gpu_scene, traversal):
    """soup1 (MaxRecursionDepth 0): the whole mixed batch, bit-identical; a miss is the
    background, as depth 0 is this scene's maximum."""
    xml = rq_util.scene_xml("soup1", scene_dir)
    b, rad, want, nbad = radiance_case(gpu_scene(xml, traversal), xml, "soup1", 0, False,
                                       f"soup1/{traversal}")
    assert nbad == 0
    miss = want[:, 3] == INF
    assert miss.sum() >= 1000 and (rad["rgb"][miss] == np.array([7, 13, 29], np.float32)).all()
    assert (want[~miss, 0:3] != 0).any(axis=1).sum() >= 1000


@pytest.mark.parametrize("traversal", MODES)
@pytest.mark.parametrize("in_medium", [False, True])
@pytest.mark.parametrize("depth", [0, 1, -1])
@pytest.mark.parametrize("name", GLASS)
def test_radiance_recursive(scene_dir, gpu_scene, name, depth, in_medium, traversal):
    """Mirror and glass scenes, the mixed batch built from their own camera-0 hits (bounce rays
    start on mirrors and inside glass): the depth argument and RT_QUERY_IN_MEDIUM against the
    oracle's Scene::trace with the same arguments.  Tolerance: the project's (assert_parity: 1
    ulp), and no differing channel at depth 0 without in_medium, where nothing recurses."""
    xml = rq_util.scene_xml(name, scene_dir)
    what = f"{name}/depth{depth}/medium{in_medium}/{traversal}"
    b, rad, want, nbad = radiance_case(gpu_scene(xml, traversal), xml, name, depth, in_medium, what)
    if depth == 0 and not in_medium:
        assert nbad == 0
    other = expected_radiance(xml, name, "mixed", depth, not in_medium)[1]
    assert (bits(other[:, 0:3]) != bits(want[:, 0:3])).any(axis=1).sum() >= 100
    if depth != 0:
        flat = expected_radiance(xml, name, "mixed", 0, in_medium)[1]
        assert (bits(flat[:, 0:3]) != bits(want[:, 0:3])).any(axis=1).sum() >= 100


# ---------------------------------------------------------------- 4. batch shape
def test_prefixes_and_untouched_tail(scene_dir, gpu_scene):
    """Prefixes of 300 rays drawn across soup1's mixed batch: each result is the oracle's for
    that ray whatever n is, and the slots past n keep their poison."""
    xml = rq_util.scene_xml("soup1", scene_dir)
    b, want = expected(xml, "soup1", "mixed")
    _, rad_want, _ = expected_radiance(xml, "soup1", "mixed", 0, False)
    pick = rb.permutation(b)[:300]
    assert len(np.unique(b.part[pick])) == len(rb.PARTS)
    o, d = b.o[pick], b.d[pick]
    s = gpu_scene(xml, "fast")
    for reorder in (False, True):
        for n in (1, 63, 64, 65, 257):
            w = SimpleNamespace(hit=want.hit[pick][:n], t=want.t[pick][:n],
                                normal=want.normal[pick][:n])
            assert not want.nan_t.any()
            hits, tail = trace(s, o, d, reorder=reorder, n=n, pad=64)
            assert_hits_match(hits, w, f"prefix {n} reorder{reorder}")
            assert len(tail) == 64 * 32 and (tail == 0xA5).all(), (n, reorder)
            rad, tail = shade_device(s, o, d, n=n, pad=64, reorder=reorder)
            assert np.array_equal(bits(rad["rgb"]), bits(rad_want[pick][:n, 0:3])), (n, reorder)
            assert np.array_equal(bits(rad["t"]), bits(rad_want[pick][:n, 3])), (n, reorder)
            assert len(tail) == 64 * 16 and (tail == 0xA5).all(), (n, reorder)
