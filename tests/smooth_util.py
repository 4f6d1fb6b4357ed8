"""Helpers of the smooth-shading tests (rt_scene_create_surface, rt_hit_attributes).

The oracle knows one normal per triangle, so the judge of a smooth scene is a restatement outside
it, in the manner of lit_util: numpy float32 arithmetic (one rounding per operation, never
contracted), the oracle's operation order, `math.pow` / `exp` / `log` for the fp64 calls.
It is HW3's smooth normal under HW2's trace_ray and HW2's Mesh, and is checked against goldens from
HW3's compiled code (tests/test_ref_hw34_host.py; DESIGN.md §4.19: HW3 itself has the other sign in
Beer's law and normalises every mesh normal once more in its identity Mesh_instance).

  vertex_normals  the HW3 loader's area-weighted vertex normals (HW3/src/Scene.cpp:690-695,
                  870-876), a sequential loop.
  barycentrics    HW2/Triangle.cpp:43-57 with Triangle.h:35-37's determinant for the oracle's hit
                  primitive; it asserts that its own t equals the oracle's bit for bit on every
                  hit, which is what earns its beta and gamma their standing.
  trace           all of Scene::trace_ray (HW2/Scene.cpp:88-196) over arrays: every closest hit
                  and shadow decision from OracleScene.intersect_rays, the normal replaced on the
                  faces of smooth meshes (HW3/src/Mesh_triangle.cpp:101-106).  It recurses per
                  batch — the mirror subset, then reflection and transmission — and keeps the
                  post order of the additions.  test_smooth_host.py earns it the right to judge:
                  with nothing smooth it equals OracleScene.shade_rays bit for bit, counters
                  included.
"""
from __future__ import annotations

import math
import os

import numpy as np

import desc_xml
import rq_util

f32 = np.float32
INF = f32(np.inf)


# ---------------------------------------------------------------- scenes
def write_spec(spec, directory, name, smooth=()):
    """The spec's XML as <name>.xml with shadingMode="smooth" on the meshes listed in `smooth`
    (0-based); SceneSpec.to_xml itself stays as it is."""
    path = os.path.join(directory, name + ".xml")
    if not os.path.exists(path):
        text = spec.to_xml()
        for m in smooth:
            old = f'    <Mesh id="{m + 1}">'
            assert text.count(old) == 1
            text = text.replace(old, f'    <Mesh id="{m + 1}" shadingMode="smooth">')
        tmp = path + ".tmp"
        with open(tmp, "w") as f:
            f.write(text)
        os.replace(tmp, path)
    return path


def mesh_flags(desc, smooth):
    flags = np.zeros(desc.d.num_meshes, np.uint8)
    flags[list(smooth)] = 1
    return flags


def _verts(verts):
    return "\n".join(" ".join(repr(float(x)) for x in v) for v in verts)


def hf_spec(width=24, height=24, num_samples=None):
    """sm_hf: heightfield_scene(8, ...) with the rig of rq_util above the field."""
    from scenes import G
    spec = G.heightfield_scene(8, width, height)
    if num_samples is not None:
        spec.cameras[0].num_samples = num_samples
    else:
        spec.cameras = list(spec.cameras) + rq_util.rig((0.05, 0.3, -4.98))
    return spec


def mixed_spec():
    """sm_mixed at 17x9: a smooth mesh (mesh 0) and a flat mesh (mesh 1) that share the middle row
    of a bumpy 4 x 3 vertex grid, a loose triangle, a sphere, four lights; everything but the
    background lies in the left half of the view, where the frame's first tile is."""
    from scenes import G
    xs, ys = (-8.0, -7.0, -6.0, -5.0), (4.0, 2.5, 1.0)
    bump = ((0.0, 0.6, -0.3, 0.4), (0.5, -0.4, 0.7, 0.1), (-0.2, 0.3, 0.0, 0.6))
    verts = [(x, y, bump[r][c]) for r, y in enumerate(ys) for c, x in enumerate(xs)]

    def quads(r):
        out = []
        for c in range(3):
            tl, tr, bl, br = 4 * r + c + 1, 4 * r + c + 2, 4 * r + c + 5, 4 * r + c + 6
            out += [f"{tl} {bl} {br}", f"{tl} {br} {tr}"]
        return "\n".join(out)

    verts += [(-4.5, 0.5, 0.2), (-1.5, 1.0, -0.1), (-3.0, 3.5, 0.4), (-3.0, -1.75, 0.0)]
    cam = G.Camera((0, 0, 5), (0, 0, -1), (0, 1, 0), (-1.7, 1.7, -0.9, 0.9), 1, 17, 9, "mixed.png")
    return G.SceneSpec(
        cameras=[cam], ambient=(20, 20, 20), background=(3, 5, 7),
        lights=[((-6.0, 3.0, 6.0), (900, 900, 900)), ((2.0, 5.0, 4.0), (600, 500, 400)),
                ((-3.0, -4.0, 5.0), (300, 400, 500)), ((-9.0, 0.0, 3.0), (400, 200, 300))],
        materials=[G.Material((1, 1, 1), (0.8, 0.6, 0.4), (0.5, 0.5, 0.5), phong=8),
                   G.Material((1, 1, 1), (0.3, 0.7, 0.5), (0.4, 0.4, 0.4), phong=3)],
        vertex_text=_verts(verts), meshes=[(1, quads(0)), (2, quads(1))],
        triangles=[(1, (13, 14, 15))], spheres=[(2, 16, 1.25)])


def icosphere(center, radius):
    """An icosahedron subdivided once (42 vertices, 80 faces), faces wound outward."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    base = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g),
            (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4),
             (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8),
             (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    unit = lambda v: tuple(x / math.sqrt(sum(y * y for y in v)) for x in v)  # noqa: E731
    pts = [unit(v) for v in base]
    mid = {}

    def midpoint(a, b):
        key = (min(a, b), max(a, b))
        if key not in mid:
            pts.append(unit(tuple((pts[a][k] + pts[b][k]) / 2 for k in range(3))))
            mid[key] = len(pts) - 1
        return mid[key]

    out = []
    for a, b, c in faces:
        ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
        out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
    fixed = []
    for a, b, c in out:
        p, q, r = (np.array(pts[k]) for k in (a, b, c))
        fixed.append((a, b, c) if np.dot(np.cross(q - p, r - p), p + q + r) > 0 else (a, c, b))
    verts = [tuple(round(center[k] + radius * v[k], 6) for k in range(3)) for v in pts]
    return verts, fixed


def glass_spec(width=33, height=31):
    """sm_glass, depth 3: an 80-face icosphere with a mirror material (mesh 0), one with glass
    (mesh 1), a flat floor (mesh 2)."""
    from scenes import G
    v0, f0 = icosphere((-1.15, 0.0, 0.0), 1.0)
    v1, f1 = icosphere((1.15, 0.0, 0.1), 1.0)
    floor = [(-4.0, -1.2, -4.0), (4.0, -1.2, -4.0), (4.0, -1.2, 4.0), (-4.0, -1.2, 4.0)]
    verts = v0 + v1 + floor
    text = lambda faces, base: "\n".join(" ".join(str(i + base + 1) for i in f) for f in faces)  # noqa: E731
    b2 = len(v0) + len(v1)
    cam = G.Camera((0.2, 1.0, 4.5), (0, -0.2, -1), (0, 1, 0), (-0.7, 0.7, -0.66, 0.66), 1, width,
                   height, "glass.png")
    return G.SceneSpec(
        cameras=[cam], ambient=(15, 15, 15), background=(10, 20, 40), max_depth=3,
        lights=[((0.0, 5.0, 4.0), (900, 900, 900)), ((-4.0, 3.0, -1.0), (500, 400, 300))],
        materials=[G.Material((1, 1, 1), (0.2, 0.2, 0.3), (0.6, 0.6, 0.6), mirror=(0.7, 0.7, 0.7),
                              phong=20),
                   G.Material((1, 1, 1), (0.05, 0.05, 0.05), (0.4, 0.4, 0.4), phong=30,
                              transparency=(0.9, 0.8, 0.7), refraction_index=1.5),
                   G.Material((1, 1, 1), (0.6, 0.7, 0.5), (0.1, 0.1, 0.1), phong=2)],
        vertex_text=_verts(verts),
        meshes=[(1, text(f0, 0)), (2, text(f1, len(v0))), (3, f"{b2 + 1} {b2 + 3} {b2 + 2}\n{b2 + 1} {b2 + 4} {b2 + 3}")])


def single_spec():
    """sm_single: one mesh of one face, so the scene's root is that triangle."""
    from scenes import G
    cam = G.Camera((0.1, 0.2, 3.0), (0, 0, -1), (0, 1, 0), (-1, 1, -1, 1), 1.5, 16, 16, "single.png")
    return G.SceneSpec(
        cameras=[cam], ambient=(10, 10, 10), background=(1, 2, 3),
        lights=[((1.0, 2.0, 4.0), (300, 300, 300))],
        materials=[G.Material((1, 1, 1), (0.7, 0.5, 0.3), (0.6, 0.6, 0.6), phong=12)],
        vertex_text=_verts([(-1.5, -1.0, 0.0), (1.75, -1.25, 0.25), (0.25, 1.5, -0.5)]),
        meshes=[(1, "1 2 3")])


CASES = {  # name -> (spec factory, smooth meshes)
    "sm_hf": (hf_spec, (0,)),
    "sm_mixed": (mixed_spec, (0,)),
    "sm_glass": (glass_spec, (0, 1)),
    "sm_single": (single_spec, (0,)),
    "sm_deep": (lambda: rq_util.deep_scene(100), (0,)),
    "sm_msaa": (lambda: hf_spec(16, 16, num_samples=4), (0,)),
}
_REFERENCE = {}


def case_xml(name, directory):
    """(xml path, smooth meshes) of a test scene."""
    factory, smooth = CASES[name]
    return write_spec(factory(), directory, name, smooth), smooth


def reference(name, directory, depth=-1, in_medium=False, smooth=None, cameras=None):
    """The scene's camera rays (rq_util.Batch, the oracle's flat answers) and `trace` of them,
    computed once per (scene, depth, medium, smooth) and shared: (batch, rgb, t, counts)."""
    xml, sm = case_xml(name, directory)
    sm = sm if smooth is None else tuple(smooth)
    key = (xml, depth, in_medium, sm, None if cameras is None else tuple(cameras))
    if key not in _REFERENCE:
        b = rq_util.oracle_batch(xml, cameras=cameras)
        rgb, t, counts = trace(xml, b.o, b.d, depth, in_medium, sm)
        for a in (rgb, t, b.o, b.d):
            a.setflags(write=False)
        _REFERENCE[key] = (b, rgb, t, counts)
    return _REFERENCE[key]


def hit_kinds(desc, shape, smooth):
    """Per ray: 'smooth', 'flat' (a face of a flat mesh), 'loose', 'sphere' or 'miss'."""
    ob = Objects(desc, smooth)
    out = np.full(len(shape), "miss", dtype=object)
    h = shape >= 0
    s = shape[h]
    kinds = np.where(~ob.tri[s], "sphere", np.where(ob.smooth[s], "smooth",
                     np.where(ob.mesh[s] >= 0, "flat", "loose")))
    out[h] = kinds
    return out


# ---------------------------------------------------------------- vector helpers
def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _length(a):
    return np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])


def _normalize(a):
    return a / _length(a)[:, None]


def _cross(a, b):  # Vector3::cross (HW3/include/Vector3.h:106-109): this = a, rhs = b
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _det(c1, c2, c3):  # Triangle.h:35-37
    return (c1[:, 0] * (c2[:, 1] * c3[:, 2] - c3[:, 1] * c2[:, 2]) +
            c2[:, 0] * (c3[:, 1] * c1[:, 2] - c1[:, 1] * c3[:, 2]) +
            c3[:, 0] * (c1[:, 1] * c2[:, 2] - c2[:, 1] * c1[:, 2]))


def _pow(c, e):
    def one(x, y):
        try:
            return math.pow(x, y)
        except (ValueError, OverflowError):
            return float(np.power(np.float64(x), np.float64(y)))
    return np.array([one(float(x), float(y)) for x, y in zip(c, e)], np.float64)


def _beer(T, t):  # (float)exp(-log((double)T) * (double)t), Scene.cpp:166-168
    def one(x, y):
        try:
            lg = math.log(x) if x != 0.0 else -math.inf
        except ValueError:
            lg = math.nan
        try:
            return math.exp(-lg * y)
        except OverflowError:
            return math.inf
    return np.array([one(float(x), float(y)) for x, y in zip(T, t)], np.float64).astype(f32)


# ---------------------------------------------------------------- vertex normals
def vertex_normals(desc):
    """(num_vertices, 3) float32: vn = 0; per mesh and face in order c = (v1 - v0) x (v2 - v0),
    n = c / |c|, area = |c| / 2, vn[i] = vn[i] + n * area for i0, i1, i2; at the end every vertex
    that got a contribution becomes vn / |vn|."""
    d, a = desc.d, desc.arrays
    v = desc.verts.reshape(-1, 3)
    vn = np.zeros((d.num_vertices, 3), f32)
    has = np.zeros(d.num_vertices, bool)
    faces = a["mesh_faces"].reshape(-1, 3)
    total = int(a["mesh_face_count"][:d.num_meshes].sum()) if d.num_meshes else 0
    two = f32(2)
    with np.errstate(all="ignore"):
        for f in range(total):
            i0, i1, i2 = (int(x) for x in faces[f])
            c = _cross(v[i1] - v[i0], v[i2] - v[i0])
            ln = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
            n = c / ln
            area = ln / two
            for i in (i0, i1, i2):
                vn[i] = vn[i] + n * area
                has[i] = True
        for i in np.flatnonzero(has):
            x = vn[i]
            vn[i] = x / np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
    assert vn.dtype == f32
    return vn


# ---------------------------------------------------------------- the objects
class Objects:
    """The description's primitives in object-list order as arrays."""

    def __init__(self, desc, smooth=()):
        objs = rq_util.object_list(desc)
        n = len(objs)
        self.tri = np.array([o[0] == "T" for o in objs], bool)
        self.idx = np.array([o[1:4] if o[0] == "T" else (0, 0, 0) for o in objs], np.int64).reshape(n, 3)
        self.mat = np.array([o[-1] for o in objs], np.int64)
        self.smooth = np.zeros(n, bool)
        self.mesh = np.full(n, -1, np.int64)
        base = 0
        for m in range(desc.d.num_meshes):
            cnt = int(desc.arrays["mesh_face_count"][m])
            self.mesh[base:base + cnt] = m
            if m in set(smooth):
                self.smooth[base:base + cnt] = True
            base += cnt
        self.verts = desc.verts.reshape(-1, 3)


def barycentrics(desc, o, d, shape, t, objects=None):
    """(beta, gamma) of rays (o, d) on the oracle's hit primitives `shape` (triangles all):
    HW2/Triangle.cpp:43-57.  `t`: the oracle's Hit_data::t; this function's own t must equal it
    bit for bit."""
    ob = objects or Objects(desc)
    assert ob.tri[shape].all()
    v0, v1, v2 = (ob.verts[ob.idx[shape, k]] for k in range(3))
    o = np.ascontiguousarray(o, f32)
    d = np.ascontiguousarray(d, f32)
    with np.errstate(all="ignore"):
        a1 = v0 - v1
        a2 = v0 - v2
        det = _det(a1, a2, d)
        b = (v0 - o) / det[:, None]
        beta = _det(b, a2, d)
        gamma = _det(a1, b, d)
        tt = _det(a1, a2, b)
    assert beta.dtype == f32 and tt.dtype == f32
    assert np.array_equal(tt.view(np.uint32), np.ascontiguousarray(t, f32).view(np.uint32)), \
        "the restated triangle test's t differs from the oracle's"
    return beta, gamma


def interpolate(x0, x1, x2, beta, gamma):
    """((x0 * w) + (x1 * beta)) + (x2 * gamma), w = (1 - beta) - gamma, per component."""
    w = (f32(1) - beta) - gamma
    return ((x0 * w[:, None]) + (x1 * beta[:, None])) + (x2 * gamma[:, None])


def smooth_normal(vn, idx, beta, gamma):
    """Mesh_triangle.cpp:101-106: the interpolated vertex normal, normalised."""
    with np.errstate(all="ignore"):
        N = interpolate(vn[idx[:, 0]], vn[idx[:, 1]], vn[idx[:, 2]], beta, gamma)
        return N / _length(N)[:, None]


# ---------------------------------------------------------------- Scene::trace_ray
class Tracer:
    """Scene::trace_ray over ray batches.  smooth: the 0-based meshes with shadingMode smooth;
    vn: their vertex normals (None: vertex_normals(desc))."""

    def __init__(self, xml, smooth=(), vn=None):
        from oracle.cpu_ref import OracleScene
        self.desc = desc = desc_xml.Desc(xml)
        self.orc = OracleScene(xml)
        self.ob = Objects(desc, smooth)
        self.vn = None
        if len(tuple(smooth)):
            self.vn = vertex_normals(desc) if vn is None else np.ascontiguousarray(vn, f32)
        self.eps = f32(desc.d.shadow_ray_epsilon)
        self.ambient = np.array(list(desc.d.ambient_light), f32)
        self.background = np.array(list(desc.d.background), f32)
        self.max_depth = int(desc.d.max_recursion_depth)
        nm = desc.d.num_materials
        fld = lambda name: np.array([list(getattr(desc.mats[m], name)) for m in range(nm)], f32)  # noqa: E731
        self.ka, self.kd, self.ks = fld("ambient"), fld("diffuse"), fld("specular")
        self.km, self.kt = fld("mirror"), fld("transparency")
        self.phong = np.array([desc.mats[m].phong_exponent for m in range(nm)], f32)
        self.index = np.array([desc.mats[m].refraction_index for m in range(nm)], f32)
        nl = desc.d.num_lights
        self.lpos = np.array([list(desc.lights[i].position) for i in range(nl)], f32).reshape(nl, 3)
        self.lint = np.array([list(desc.lights[i].intensity) for i in range(nl)], f32).reshape(nl, 3)
        self.counts = {"primary_rays": 0, "primary_hits": 0, "shadow_rays": 0, "secondary_rays": 0}

    def close(self):
        self.orc.close()

    def hit_normals(self, o, d, rec, shape, idx):
        """Hit_data::normal of the hits `idx`: the oracle's, replaced on smooth faces."""
        nrm = rec[idx, 4:7].copy()
        sm = self.ob.smooth[shape[idx]]
        if sm.any():
            k = idx[sm]
            beta, gamma = barycentrics(self.desc, o[k], d[k], shape[k], rec[k, 3], self.ob)
            nrm[sm] = smooth_normal(self.vn, self.ob.idx[shape[k]], beta, gamma)
        return nrm

    @staticmethod
    def _refract(dr, n, idx):  # HW2/Scene.cpp:72-86
        n_ratio = f32(1) / idx
        cos_t = _dot(-dr, n)
        delta = f32(1) - (n_ratio * n_ratio) * (f32(1) - (cos_t * cos_t))
        ok = ~(delta < f32(0))
        out = _normalize((dr + n * cos_t[:, None]) * n_ratio[:, None] - n * np.sqrt(delta)[:, None])
        return ok, out

    def trace(self, o, d, medium, depth):
        """Colours (n, 3) and first-hit t (n,) of rays (o, d, medium[i]) at `depth`."""
        n = len(o)
        color = np.zeros((n, 3), f32)
        t_out = np.full(n, INF, f32)
        if n == 0:
            return color, t_out
        rec, shape = self.orc.intersect_rays(o, d)
        hit = rec[:, 7] == 1.0
        if depth == self.max_depth:
            color[~hit] = self.background
            self.counts["primary_hits"] += int(hit.sum())
        idx = np.flatnonzero(hit)
        if not len(idx):
            return color, t_out
        t = rec[idx, 3]
        t_out[idx] = t
        nrm = self.hit_normals(o, d, rec, shape, idx)
        mat = self.ob.mat[shape[idx]]
        oh, dh = o[idx], d[idx]
        p = oh + dh * t[:, None]
        w0 = _normalize(oh - p)
        c = np.zeros((len(idx), 3), f32)
        lit = np.flatnonzero(~medium[idx])
        if len(lit):
            c[lit] = c[lit] + self.ka[mat[lit]] * self.ambient[None, :]
            for j in range(len(self.lpos)):
                self._light(c, lit, p, nrm, w0, mat, self.lpos[j][None, :], self.lint[j][None, :])
        depth_ok = depth > 0
        # mirror (Scene.cpp:141-146)
        wr = _normalize(nrm * (f32(2) * _dot(nrm, w0))[:, None] - w0)
        a = np.flatnonzero((self.km[mat] != 0).any(axis=1)) if depth_ok else np.zeros(0, np.int64)
        if len(a):
            self.counts["secondary_rays"] += len(a)
            sub, _ = self.trace(p[a] + wr[a] * self.eps, wr[a], np.zeros(len(a), bool), depth - 1)
            c[a] = c[a] + self.km[mat[a]] * sub
        # dielectric (Scene.cpp:149-194)
        g = np.flatnonzero((self.kt[mat] != 0).any(axis=1)) if depth_ok else np.zeros(0, np.int64)
        if len(g):
            ng, pg, wrg = nrm[g], p[g], wr[g]
            dn = _normalize(dh[g])
            ior = self.index[mat[g]]
            entering = _dot(dn, ng) < f32(0)
            k = np.ones((len(g), 3), f32)
            ok_in, td_in = self._refract(dn, ng, ior)
            cos_in = _dot(-dn, ng)
            T = self.kt[mat[g]]
            kout = np.stack([_beer(T[:, ch], t[g]) for ch in range(3)], axis=1)
            ok_out, td_out = self._refract(dn, -ng, f32(1) / ior)
            cos_out = _dot(td_out, ng)
            k = np.where(entering[:, None], k, kout).astype(f32)
            td = np.where(entering[:, None], np.where(ok_in[:, None], td_in, f32(0)), td_out).astype(f32)
            cos_t = np.where(entering, cos_in, cos_out).astype(f32)
            tir = ~entering & ~ok_out
            q = np.flatnonzero(tir)
            if len(q):
                self.counts["secondary_rays"] += len(q)
                sub, _ = self.trace(pg[q] + wrg[q] * self.eps, wrg[q], np.ones(len(q), bool), depth - 1)
                c[g[q]] = c[g[q]] + k[q] * sub
            q = np.flatnonzero(~tir)
            if len(q):
                iq = ior[q]
                r0 = (iq - f32(1)) * (iq - f32(1)) / ((iq + f32(1)) * (iq + f32(1)))
                r = (r0.astype(np.float64) + (f32(1) - r0).astype(np.float64) *
                     _pow(f32(1) - cos_t[q], np.full(len(q), 5.0))).astype(f32)
                self.counts["secondary_rays"] += 2 * len(q)
                ent = entering[q]
                refl, _ = self.trace(pg[q] + wrg[q] * self.eps, wrg[q], ~ent, depth - 1)
                tran, _ = self.trace(pg[q] + td[q] * self.eps, td[q], ent.copy(), depth - 1)
                A = refl * r[:, None]
                B = tran * (f32(1) - r)[:, None]
                c[g[q]] = c[g[q]] + k[q] * (A + B)
        color[idx] = c
        return color, t_out

    def _light(self, c, lit, p, nrm, w0, mat, lpos, lint):
        """One light of the loop (Scene.cpp:113-138) for the shading hits `lit`."""
        pa = p[lit]
        ld = lpos - pa
        dist = _length(ld)
        wi = ld / dist[:, None]
        srec, _ = self.orc.intersect_rays(pa + wi * self.eps, wi)
        self.counts["shadow_rays"] += len(lit)
        st = srec[:, 3]
        occ = (srec[:, 7] == 1.0) & (st < (dist - self.eps)) & (st > f32(0))
        d2 = dist * dist
        cos_d = _dot(nrm[lit], wi)
        m = mat[lit]
        dif = ((self.kd[m] * lint) * cos_d[:, None]) / d2[:, None]
        hv = w0[lit] + wi
        cos_s = np.fmax(_dot(nrm[lit], _normalize(hv)), f32(0))
        pw = _pow(cos_s, self.phong[m]).astype(f32)
        spe = ((self.ks[m] * lint) * pw[:, None]) / d2[:, None]
        on = lit[~occ]
        c[on] = (c[on] + dif[~occ]) + spe[~occ]


def trace(xml, o, d, depth=-1, in_medium=False, smooth=(), vn=None):
    """Scene::trace_ray(Ray(o, d, in_medium), depth) of every ray; depth -1: the scene's maximum.
    Returns ((n, 3) colours as a zeroed Pixel holds them, (n,) first-hit t or +inf, ray counts)."""
    tr = Tracer(xml, smooth, vn)
    o = np.ascontiguousarray(o, f32)
    d = np.ascontiguousarray(d, f32)
    if depth < 0:
        depth = tr.max_depth
    with np.errstate(all="ignore"):
        color, t = tr.trace(o, d, np.full(len(o), bool(in_medium)), depth)
    tr.counts["primary_rays"] = len(o)
    tr.close()
    out = f32(0) + color
    assert out.dtype == f32 and t.dtype == f32
    return out, t, tr.counts


def restate_lit(xml, o, d, own, smooth=(), vn=None):
    """lit_util.restate (the depth-0 shading with the caller's light records `own`) with
    Hit_data::normal replaced on the faces of smooth meshes.  lit_util takes its hits from
    OracleScene.intersect_rays; for the length of the call that class answers the query of the
    primary rays themselves — recognised by its origins and directions being (o, d), not by its
    place among the calls — with the smooth normals, and the shadow-ray queries as they are.  It
    must have done so exactly once."""
    import lit_util
    import oracle.cpu_ref as cpu_ref
    o = np.ascontiguousarray(o, f32)
    d = np.ascontiguousarray(d, f32)
    tr = Tracer(xml, smooth, vn)
    plain = cpu_ref.OracleScene
    replaced = []

    class SmoothNormals(plain):
        def intersect_rays(self, origins, directions):
            rec, shape = super().intersect_rays(origins, directions)
            qo, qd = np.asarray(origins, f32), np.asarray(directions, f32)
            if qo.shape == o.shape and np.array_equal(qo.view(np.uint32), o.view(np.uint32)) and \
                    np.array_equal(qd.view(np.uint32), d.view(np.uint32)):
                idx = np.flatnonzero(rec[:, 7] == 1.0)
                rec[idx, 4:7] = tr.hit_normals(o, d, rec, shape, idx)
                replaced.append(len(idx))
            return rec, shape

    cpu_ref.OracleScene = SmoothNormals
    try:
        out = lit_util.restate(xml, o, d, own)
    finally:
        cpu_ref.OracleScene = plain
        tr.close()
    assert len(replaced) == 1, "the primary rays' query was not seen exactly once"
    return out
