"""The triangle test where its 2x2 minors are exactly zero (rt_kernels.hip tri_test).

Of the minors of the triangle test's four determinants that hold b = (v0 - o) / det, three —
b2 = d.y b.z - b.y d.z, b3 = b.y a2.z - a2.y b.z, g3 = a1.y b.z - b.y a1.z — occur twice, once
mirrored (y x' - x y' for x y' - y x').  A non-zero difference has the same bits either way; an
exact zero has a sign, and what the compiler or a rewrite shares of these minors decides which one
(round 18 built the shared, negated form: DESIGN.md §4.3).  The sign must never show: the values
are only compared, and a hit's t is positive.

Scene: 16 axis-aligned and 16 tilted triangles on a grid of eighths (every product and sum below
is then exact where it matters).  4,200 query rays in five families: directions along one axis
(three in four +-x, where b2 = 0 for every triangle); origins that share two coordinates with a
triangle's first vertex (y and z: b.y = b.z = +-0 and all three minors vanish); rays inside a
triangle's plane (det = 0); rays through a vertex; rays along an edge.  The CPU part evaluates the
three minors for every ray and triangle in fp32 as the kernel orders them and states the share of
rays with an exactly-zero shared minor, which must be at least half; the GPU part compares
rt_trace_rays (hit, t bits, object) and rt_occluded with the CPU oracle."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_scene as G  # noqa: E402
from rq_util import bits, occlusion, trace  # noqa: E402

F = np.float32
N_FAMILY = (1400, 1400, 500, 450, 450)
FAMILIES = ("axis", "two coordinates", "in plane", "vertex", "edge")


def grid(rng, lo, hi, size=None):
    """Multiples of 1/8 in [lo, hi]."""
    return rng.integers(int(lo * 8), int(hi * 8) + 1, size).astype(np.float64) / 8


@functools.lru_cache(maxsize=None)
def triangles():
    """(32, 3, 3) vertices: 16 triangles in planes x, y or z = c with legs along the other two
    axes, then 16 tilted ones."""
    rng = np.random.default_rng(18)
    tri = []
    for i in range(16):
        p = grid(rng, -3, 2, 3)
        u, v = [(1, 2), (2, 0), (0, 1)][i % 3]
        s, t = grid(rng, 0.5, 1.5), grid(rng, 0.5, 1.5)
        e1, e2 = np.zeros(3), np.zeros(3)
        e1[u], e2[v] = s, t
        tri.append([p, p + e1, p + e2])
    while len(tri) < 32:
        p = grid(rng, -3, 2, 3)
        e1, e2 = grid(rng, -1.5, 1.5, 3), grid(rng, -1.5, 1.5, 3)
        n = np.cross(e1, e2)
        if (np.abs(n) > 0.1).all():  # tilted against every axis
            tri.append([p, p + e1, p + e2])
    return np.array(tri)


def spec():
    T = triangles()
    verts = T.reshape(-1, 3)
    return G.SceneSpec(
        cameras=[G.Camera((0, 0, 8), (0, 0, -1), (0, 1, 0), (-1, 1, -1, 1), 2, 16, 16, "zm.png")],
        ambient=(20, 20, 20), lights=[((1.0, 6.0, 5.0), (300, 300, 300))],
        materials=[G.Material((1, 1, 1), (0.8, 0.6, 0.4), (0.2, 0.2, 0.2), phong=4)],
        vertex_text="\n".join(" ".join(repr(float(x)) for x in v) for v in verts),
        triangles=[(1, (3 * k + 1, 3 * k + 2, 3 * k + 3)) for k in range(len(T))])


def scene_xml(directory):
    path = os.path.join(directory, "tri_zero_minors.xml")
    if not os.path.exists(path):
        with open(path, "w") as f:
            f.write(spec().to_xml())
    return path


def skew_triangles():
    """The triangles whose edge vectors v0 - v1 and v0 - v2 have no zero y or z component."""
    T = triangles()
    a1, a2 = T[:, 0] - T[:, 1], T[:, 0] - T[:, 2]
    k = np.nonzero(((a1[:, 1:] != 0) & (a2[:, 1:] != 0)).all(axis=1))[0]
    assert len(k) >= 8 and (k >= 16).all()
    return k


@functools.lru_cache(maxsize=None)
def rays():
    """(o, d, family index), fp32; every coordinate a multiple of 1/8 (or of 1/64: the in-plane
    and edge points), so v0 - o, the edge vectors and the directions are exact."""
    T = triangles()
    rng = np.random.default_rng(795)
    o, d = [], []
    skew = skew_triangles()
    # directions along one axis: three in four +-x, the rest +-y and +-z
    for i in range(N_FAMILY[0]):
        axis = 0 if i % 4 else 1 + (i // 4) % 2
        k = rng.integers(len(T))
        c = T[k].mean(axis=0) if i % 3 else T[k][rng.integers(3)]  # towards the inside / a vertex
        p = np.round(c * 8) / 8 if i % 3 else c.copy()
        sign = 1 if (i // 4) % 2 else -1
        p[axis] -= sign * grid(rng, 1, 5)
        e = np.zeros(3)
        e[axis] = sign * [1.0, 0.5, 2.0][i % 3]
        o.append(p)
        d.append(e)
    # origins sharing two coordinates with a first vertex — of a triangle without an axis-aligned
    # edge — y and z (seven of eight), else x and y
    for i in range(N_FAMILY[1]):
        k = skew[rng.integers(len(skew))]
        v0 = T[k][0]
        p = v0.copy()
        free = 0 if i % 8 else 2
        p[free] += rng.choice([-1, 1]) * grid(rng, 1, 4)
        target = T[k].mean(axis=0) if i % 2 else T[rng.integers(len(T))].mean(axis=0)
        o.append(p)
        d.append(np.round((target - p) * 8) / 8)
    # inside a triangle's plane: origin and direction combinations of its edges
    for i in range(N_FAMILY[2]):
        k = rng.integers(len(T))
        v0, e1, e2 = T[k][0], T[k][1] - T[k][0], T[k][2] - T[k][0]
        a, b = grid(rng, -2, 2, 2)
        p = v0 + a * e1 + b * e2
        a, b = grid(rng, -1, 1, 2)
        e = a * e1 + b * e2
        if not e.any():
            e = e1
        o.append(p)
        d.append(e)
    # through a vertex
    for i in range(N_FAMILY[3]):
        k = rng.integers(len(T))
        v = T[k][rng.integers(3)]
        p = grid(rng, -4, 4, 3)
        if (p == v).all():
            p[0] += 1
        o.append(p)
        d.append(v - p)
    # along an edge, from a point on its line
    for i in range(N_FAMILY[4]):
        k = rng.integers(len(T))
        j = rng.integers(3)
        v, w = T[k][j], T[k][(j + 1) % 3]
        o.append(v - grid(rng, 1, 3) * (w - v))
        d.append((w - v) * [1.0, 0.5, 2.0][i % 3])
    o, d = np.array(o, np.float64), np.array(d, np.float64)
    assert np.array_equal(o.astype(F), o) and np.array_equal(d.astype(F), d)  # exact in fp32
    assert d.any(axis=1).all()
    fam = np.repeat(np.arange(len(FAMILIES)), N_FAMILY)
    o, d = o.astype(F), d.astype(F)
    for a in (o, d, fam):
        a.setflags(write=False)
    return o, d, fam


@functools.lru_cache(maxsize=None)
def zero_minors():
    """Per ray: some triangle has an exactly zero b2, b3 or g3 — fp32, every product and difference
    rounded, b = (v0 - o) / det with the kernel's det (a true division; det = 0 gives inf or NaN,
    which is no zero)."""
    T = triangles().astype(F)
    o, d, _ = rays()
    v0, a1, a2 = T[:, 0][None], (T[:, 0] - T[:, 1])[None], (T[:, 0] - T[:, 2])[None]
    dd = d[:, None, :]
    with np.errstate(all="ignore"):
        m1 = a2[..., 1] * dd[..., 2] - dd[..., 1] * a2[..., 2]
        m2 = dd[..., 1] * a1[..., 2] - a1[..., 1] * dd[..., 2]
        m3 = a1[..., 1] * a2[..., 2] - a2[..., 1] * a1[..., 2]
        det = (a1[..., 0] * m1 + a2[..., 0] * m2) + dd[..., 0] * m3
        b = (v0 - o[:, None, :]) / det[..., None]
        b2 = dd[..., 1] * b[..., 2] - b[..., 1] * dd[..., 2]
        b3 = b[..., 1] * a2[..., 2] - a2[..., 1] * b[..., 2]
        g3 = a1[..., 1] * b[..., 2] - b[..., 1] * a1[..., 2]
    assert b2.dtype == F and det.dtype == F
    zero = (b2 == 0) | (b3 == 0) | (g3 == 0)
    # ... counted on the triangles whose edge vectors have no zero y or z component alone: there a
    # zero minor is the ray's doing (an axis-aligned edge makes b3 or g3 zero for every ray)
    skew = np.zeros(len(T), bool)
    skew[skew_triangles()] = True
    return (zero & skew[None]).any(axis=1), (det == 0).any(axis=1)


@functools.lru_cache(maxsize=None)
def oracle(xml):
    """(records, object index, tmax, occluded): tmax twice and half the oracle's t in turn, +inf
    on a miss."""
    from oracle.cpu_ref import OracleScene
    o, d, _ = rays()
    orc = OracleScene(xml)
    rec, obj = orc.intersect_rays(o, d)
    orc.close()
    hit, t = rec[:, 7] == 1.0, rec[:, 3]
    tmax = np.where(hit, np.where(np.arange(len(o)) % 2 == 0, t * F(2), t * F(0.5)),
                    F(np.inf)).astype(F)
    occ = (hit & (t > 0) & (t < tmax)).astype(np.uint8)
    for a in (rec, obj, tmax, occ):
        a.setflags(write=False)
    return rec, obj, tmax, occ


def case(directory):
    xml = scene_xml(directory)
    o, d, fam = rays()
    zero, flat = zero_minors()
    rec, obj, _, occ = oracle(xml)
    hit = rec[:, 7] == 1.0
    share = float(zero.mean())
    per = {FAMILIES[k]: (round(float(zero[fam == k].mean()), 3), int(hit[fam == k].sum()))
           for k in range(len(FAMILIES))}
    print(f"{len(o)} rays, {share:.3f} with an exactly zero shared minor, {int(flat.sum())} with a "
          f"zero det, {int(hit.sum())} hit; per family (share, hits): {per}")
    assert len(o) == sum(N_FAMILY) == 4200
    assert share >= 0.5
    assert zero[fam == 1].mean() >= 0.7 and flat[fam == 2].all()
    assert hit.any() and not hit.all() and hit[zero].any() and not hit[zero].all()
    assert all(h > 0 for _, h in per.values())
    assert occ.any() and not occ.all()
    assert ((obj >= 0) == hit).all()
    return xml


def test_cases_occur(scene_dir):
    case(scene_dir)


@pytest.mark.gpu
@pytest.mark.parametrize("traversal", ["fast", "reference"])
def test_closest_hit(scene_dir, traversal):
    import ceng795_amd
    xml = case(scene_dir)
    o, d, _ = rays()
    rec, obj, _, _ = oracle(xml)
    hit = rec[:, 7] == 1.0
    with ceng795_amd.Scene(xml, traversal=traversal) as s:
        hits, _ = trace(s, o, d)
    got = hits["leaf"] >= 0
    print(f"{traversal}: {len(o)} rays, {int(hit.sum())} hit, {int((got != hit).sum())} differ in "
          f"hit, {int((bits(hits['t'][hit & got]) != bits(rec[hit & got, 3])).sum())} in t")
    assert np.array_equal(got, hit)
    assert np.array_equal(bits(hits["t"][hit]), bits(rec[hit, 3]))
    assert np.array_equal(hits["object"], obj)
    assert (bits(hits["t"][~hit]) == bits(F(np.inf))).all()


@pytest.mark.gpu
@pytest.mark.parametrize("traversal", ["fast", "reference"])
def test_occlusion(scene_dir, traversal):
    import ceng795_amd
    xml = case(scene_dir)
    o, d, _ = rays()
    _, _, tmax, want = oracle(xml)
    with ceng795_amd.Scene(xml, traversal=traversal) as s:
        got, _ = occlusion(s, o, d, tmax)
    print(f"{traversal}: {int(want.sum())} occluded, {int((got != want).sum())} differ")
    assert np.array_equal(got, want)
