"""Helpers of the texture tests (rt_scene_create_textured, rt_texture_lookup*).

The oracle knows no textures, so the judge is a restatement outside it, in the manner of
smooth_util and lit_util: numpy float32 arithmetic (one rounding per operation, never contracted),
checked against goldens from the HW4 sources' compiled code (tests/test_ref_hw34_host.py; DESIGN.md
§4.19 names the departures: Beer's sign, the normals of plain meshes and spheres, the read past the
image, and textured loose triangles, which HW4 does not have).

  lookup       Texture::get_color_at (HW4/src/Texture.cpp:57-134), scalar fp32 steps in its order.
  sphere_uv    Sphere.cpp:100-105 with np.arccos / np.arctan2 on float64; also whether one of its
               fp64 values lies within 4 fp64 ulps of an fp32 rounding boundary.
  triangle_uv  Mesh_triangle.cpp:107-111.
  TexTracer    smooth_util.Tracer (closest hits and shadow decisions from the oracle, normals from
               smooth_util) with HW4's texture step at each hit (HW4/src/Scene.cpp:149-171): the
               diffuse colour of the light loop and the REPLACE_ALL rule come from here.  It counts
               shadow and secondary rays, and notes where textured hits were seen.
  restate_lit  the depth-0 shading with the caller's light records (lit_util.restate's terms) and
               the textured diffuse colour in both of them.
"""
from __future__ import annotations

import numpy as np

import desc_xml
import rq_util
import smooth_util as su
from smooth_util import _dot, _length, _normalize, _pow, _beer, f32, INF

NEAREST, BILINEAR = 0, 1
REPLACE_KD, BLEND_KD, REPLACE_ALL = 0, 1, 2
REPEAT, CLAMP = 0, 1


def texture(rgb8, interpolation=BILINEAR, decal=BLEND_KD, appearance=CLAMP, normalizer=255.0):
    return dict(rgb8=np.ascontiguousarray(rgb8, np.uint8), interpolation=interpolation,
                decal=decal, appearance=appearance, normalizer=normalizer)


def random_texture(w, h, seed, **kw):
    """A seeded (h, w, 3) uint8 image."""
    return texture(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8), **kw)


# ---------------------------------------------------------------- Texture::get_color_at
def _fmin(a, b):  # C fmin: the operand that is not NaN
    return b if np.isnan(a) else a if np.isnan(b) else (a if a < b else b)


def _fmax(a, b):
    return b if np.isnan(a) else a if np.isnan(b) else (a if a > b else b)


def lookup(tex, u, v):
    """Texture::get_color_at(u, v): (3,) float32 raw channel values.  Texture.cpp line numbers on
    the right.  The one departure of the contract: a term of the clamped bilinear form whose linear
    texel index is >= w * h is skipped (the reference reads past its buffer there)."""
    img = tex["rgb8"]
    h, w = int(img.shape[0]), int(img.shape[1])
    flat = img.reshape(-1, 3)  # the reference's linear addressing, 3 * (w * row + column)
    one, zero = f32(1), f32(0)
    u, v = f32(u), f32(v)
    with np.errstate(all="ignore"):
        if tex["appearance"] == CLAMP:                       # :58-60
            u = _fmax(zero, _fmin(one, u))
            v = _fmax(zero, _fmin(one, v))
        else:                                                # :62-63
            u = _fmax(zero, _fmin(one, f32(u - np.floor(u))))
            v = _fmax(zero, _fmin(one, f32(v - np.floor(v))))
        u = f32(u * f32(w))                                  # :65-68
        if u >= f32(w):
            u = f32(u - one)
        v = f32(v * f32(h))
        if v >= f32(h):
            v = f32(v - one)
        if tex["interpolation"] == NEAREST:                  # :71-74
            return flat[w * int(v) + int(u)].astype(f32)
        if tex["appearance"] == REPEAT:                      # :77-100
            p = int(u) % w
            pn = (p + 1) % w
            q = int(v) % h
            qn = (q + 1) % h
            dx, dy = f32(u - f32(p)), f32(v - f32(q))
            c = f32(f32(flat[w * q + p].astype(f32) * f32(one - dx)) * f32(one - dy))
            c = f32(c + f32(f32(flat[w * q + pn].astype(f32) * dx) * f32(one - dy)))
            c = f32(c + f32(f32(flat[w * qn + pn].astype(f32) * dx) * dy))
            c = f32(c + f32(f32(flat[w * qn + p].astype(f32) * f32(one - dx)) * dy))
            return np.asarray(c, f32)
        p = int(u)                                           # :102-129
        pn = p + 1
        q = int(v)
        qn = int(f32(v + one))
        dx, dy = f32(u - f32(p)), f32(v - f32(q))
        c = f32(f32(flat[w * q + p].astype(f32) * f32(one - dx)) * f32(one - dy))
        if pn < w:
            c = f32(c + f32(f32(flat[w * q + pn].astype(f32) * dx) * f32(one - dy)))
        if qn < h and w * qn + pn < w * h:                   # (the departure: no read past the end)
            c = f32(c + f32(f32(flat[w * qn + pn].astype(f32) * dx) * dy))
        if pn < w and qn < h:
            c = f32(c + f32(f32(flat[w * qn + p].astype(f32) * f32(one - dx)) * dy))
        return np.asarray(c, f32)


def lookups(tex, u, v):
    """lookup over arrays: (n, 3) float32."""
    out = np.zeros((len(u), 3), f32)
    for i, (a, b) in enumerate(zip(u, v)):
        out[i] = lookup(tex, a, b)
    assert out.dtype == f32
    return out


def pn_equals_w(tex, u):
    """Does a clamped bilinear lookup at `u` have pn == w?"""
    w = int(tex["rgb8"].shape[1])
    x = _fmax(f32(0), _fmin(f32(1), f32(u)))
    x = f32(x * f32(w))
    if x >= f32(w):
        x = f32(x - f32(1))
    return int(x) + 1 == w


def edge_coordinates(n):
    """The grid of the lookup tests for a side of n texels: k / n and its two fp32 neighbours for
    k = 0 .. n, and the values the clamps, the wrap and the NaN rule are for."""
    out = []
    for k in range(n + 1):
        x = f32(k) / f32(n)
        out += [np.nextafter(x, f32(-np.inf)), x, np.nextafter(x, f32(np.inf))]
    out += [-0.0, -0.25, -1.0, 1.0 - 2.0 ** -24, 1.0, 1.5, 2.0, 1e9, np.nan, np.inf, -np.inf]
    return np.array(out, f32)


# ---------------------------------------------------------------- (u, v) of a hit
def _near_boundary(x64):
    """Is the float64 x within 4 fp64 ulps of a point where its rounding to fp32 changes?"""
    x64 = np.asarray(x64, np.float64)
    f = x64.astype(f32)
    near = np.zeros(x64.shape, bool)
    for side in (-np.inf, np.inf):
        nb = np.nextafter(f, f32(side)).astype(np.float64)
        mid = (f.astype(np.float64) + nb) / 2.0
        near |= np.abs(x64 - mid) <= 4.0 * np.spacing(np.abs(x64))
    return near


def sphere_uv(lc, radius):
    """Sphere.cpp:100-105 for local points lc (n, 3) float32 = hit point - center: (u, v) float32
    and, per point, whether theta, phi, u or v lies near an fp32 rounding boundary as a float64."""
    lc = np.ascontiguousarray(lc, f32)
    with np.errstate(all="ignore"):
        c = (lc[:, 1] / f32(radius)).astype(np.float64)
        theta64 = np.arccos(c)
        theta = theta64.astype(f32)
        phi64 = np.arctan2(lc[:, 2].astype(np.float64), lc[:, 0].astype(np.float64))
        phi = phi64.astype(f32)
        u64 = (np.pi - phi.astype(np.float64)) / (2 * np.pi)
        v64 = theta.astype(np.float64) / np.pi
    near = _near_boundary(theta64) | _near_boundary(phi64) | _near_boundary(u64) | _near_boundary(v64)
    return u64.astype(f32), v64.astype(f32), near


def triangle_uv(uva, uvb, uvc, beta, gamma):
    """Mesh_triangle.cpp:107-111: (a + beta * (b - a)) + gamma * (c - a) per component."""
    b, g = beta[:, None], gamma[:, None]
    out = (uva + b * (uvb - uva)) + g * (uvc - uva)
    assert out.dtype == f32
    return out[:, 0], out[:, 1]


# ---------------------------------------------------------------- Scene::trace_ray with textures
class TexTracer(su.Tracer):
    """smooth_util.Tracer plus textures: `textures` a list of texture() dicts, the three per-object
    id lists (None: none), `uv` the (num_vertices, 2) float32 texture coordinates."""

    def __init__(self, xml, textures=(), mesh_texture=None, triangle_texture=None,
                 sphere_texture=None, uv=None, smooth=(), vn=None):
        super().__init__(xml, smooth, vn)
        d = self.desc.d
        self.textures = list(textures)
        self.uv = None if uv is None else np.ascontiguousarray(uv, f32).reshape(-1, 2)
        ids = []
        faces = self.desc.arrays["mesh_face_count"]
        for m in range(d.num_meshes):
            ids += [-1 if mesh_texture is None else int(mesh_texture[m])] * int(faces[m])
        ids += [-1 if triangle_texture is None else int(triangle_texture[k])
                for k in range(d.num_triangles)]
        ids += [-1 if sphere_texture is None else int(sphere_texture[k])
                for k in range(d.num_spheres)]
        self.obj_tex = np.array(ids, np.int64)
        assert len(self.obj_tex) == len(self.ob.tri)
        objs = rq_util.object_list(self.desc)
        self.center = np.zeros((len(objs), 3), f32)
        self.radius = np.zeros(len(objs), f32)
        for k, o in enumerate(objs):
            if o[0] == "S":
                self.center[k] = np.array(o[1:4], np.uint32).view(f32)
                self.radius[k] = np.array(o[4:5], np.uint32).view(f32)[0]
        # what the scene's rays met: (decal or "sphere" / "pn==w", how the ray came about) pairs
        self.seen = set()
        self.lookups = []  # (texture id, u, v) of every lookup, in order

    def texture_step(self, o, d, rec, shape, idx, p, via):
        """HW4/src/Scene.cpp:154-170 for the hits `idx`: (kd (n, 3), replace_all (n,), the raw
        texel (n, 3), near (n,): a sphere hit whose (u, v) sits near a rounding boundary)."""
        mat = self.ob.mat[shape[idx]]
        kd = self.kd[mat].copy()
        n = len(idx)
        rall = np.zeros(n, bool)
        texel = np.zeros((n, 3), f32)
        near = np.zeros(n, bool)
        tid = self.obj_tex[shape[idx]]
        tx = np.flatnonzero(tid >= 0)
        if not len(tx):
            self.seen.add(("untextured", via))
            return kd, rall, texel, near
        if (tid < 0).any():
            self.seen.add(("untextured", via))
        u = np.zeros(n, f32)
        v = np.zeros(n, f32)
        sh = shape[idx]
        tri = tx[self.ob.tri[sh[tx]]]
        if len(tri):
            k = idx[tri]
            beta, gamma = su.barycentrics(self.desc, o[k], d[k], shape[k], rec[k, 3], self.ob)
            vi = self.ob.idx[shape[k]]
            u[tri], v[tri] = triangle_uv(self.uv[vi[:, 0]], self.uv[vi[:, 1]], self.uv[vi[:, 2]],
                                         beta, gamma)
        sph = tx[~self.ob.tri[sh[tx]]]
        for r in np.unique(self.radius[sh[sph]]) if len(sph) else ():
            s = sph[self.radius[sh[sph]] == r]
            lc = p[s] - self.center[sh[s]]
            u[s], v[s], near[s] = sphere_uv(lc, r)
            self.seen.add(("sphere", via))
        for i in tx:
            t = self.textures[tid[i]]
            texel[i] = lookup(t, u[i], v[i])
            self.lookups.append((int(tid[i]), u[i], v[i]))
            self.seen.add((t["decal"], via))
            if t["interpolation"] == BILINEAR and t["appearance"] == CLAMP and pn_equals_w(t, u[i]):
                self.seen.add(("pn==w", via))
            if t["decal"] == REPLACE_ALL:
                rall[i] = True
            else:
                tc = texel[i] / f32(t["normalizer"])  # Scene.cpp:166
                kd[i] = tc if t["decal"] == REPLACE_KD else (tc + kd[i]) / f32(2)  # Texture.cpp:46-50
        assert kd.dtype == f32 and texel.dtype == f32
        return kd, rall, texel, near

    def trace(self, o, d, medium, depth, via="primary"):
        """Colours (n, 3), first-hit t (n,) and, per ray, whether some sphere lookup of its tree
        sits near a rounding boundary."""
        n = len(o)
        color = np.zeros((n, 3), f32)
        t_out = np.full(n, INF, f32)
        flag = np.zeros(n, bool)
        if n == 0:
            return color, t_out, flag
        rec, shape = self.orc.intersect_rays(o, d)
        hit = rec[:, 7] == 1.0
        if depth == self.max_depth:
            color[~hit] = self.background
            self.counts["primary_hits"] += int(hit.sum())
        if (~hit).any():
            self.seen.add(("miss", via))
        idx = np.flatnonzero(hit)
        if not len(idx):
            return color, t_out, flag
        t = rec[idx, 3]
        t_out[idx] = t
        nrm = self.hit_normals(o, d, rec, shape, idx)
        mat = self.ob.mat[shape[idx]]
        oh, dh = o[idx], d[idx]
        p = oh + dh * t[:, None]
        w0 = _normalize(oh - p)
        kd, rall, texel, near = self.texture_step(o, d, rec, shape, idx, p, via)
        f = near.copy()
        c = np.zeros((len(idx), 3), f32)
        c[rall] = texel[rall]                                # Scene.cpp:156-159: nothing else
        lit = np.flatnonzero(~medium[idx] & ~rall)
        if len(lit):
            c[lit] = c[lit] + self.ka[mat[lit]] * self.ambient[None, :]
            for j in range(len(self.lpos)):
                self._light(c, lit, p, nrm, w0, mat, self.lpos[j][None, :], self.lint[j][None, :], kd)
        depth_ok = depth > 0
        none = np.zeros(0, np.int64)
        wr = _normalize(nrm * (f32(2) * _dot(nrm, w0))[:, None] - w0)
        a = np.flatnonzero((self.km[mat] != 0).any(axis=1) & ~rall) if depth_ok else none
        if len(a):
            self.counts["secondary_rays"] += len(a)
            sub, _, sf = self.trace(p[a] + wr[a] * self.eps, wr[a], np.zeros(len(a), bool), depth - 1,
                                    "mirror")
            c[a] = c[a] + self.km[mat[a]] * sub
            f[a] |= sf
        g = np.flatnonzero((self.kt[mat] != 0).any(axis=1) & ~rall) if depth_ok else none
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
                sub, _, sf = self.trace(pg[q] + wrg[q] * self.eps, wrg[q], np.ones(len(q), bool),
                                        depth - 1, "tir")
                c[g[q]] = c[g[q]] + k[q] * sub
                f[g[q]] |= sf
            q = np.flatnonzero(~tir)
            if len(q):
                iq = ior[q]
                r0 = (iq - f32(1)) * (iq - f32(1)) / ((iq + f32(1)) * (iq + f32(1)))
                r = (r0.astype(np.float64) + (f32(1) - r0).astype(np.float64) *
                     _pow(f32(1) - cos_t[q], np.full(len(q), 5.0))).astype(f32)
                self.counts["secondary_rays"] += 2 * len(q)
                ent = entering[q]
                refl, _, rf = self.trace(pg[q] + wrg[q] * self.eps, wrg[q], ~ent, depth - 1,
                                         "reflection")
                tran, _, tf = self.trace(pg[q] + td[q] * self.eps, td[q], ent.copy(), depth - 1,
                                         "transmission")
                A = refl * r[:, None]
                B = tran * (f32(1) - r)[:, None]
                c[g[q]] = c[g[q]] + k[q] * (A + B)
                f[g[q]] |= rf | tf
        color[idx] = c
        flag[idx] = f
        return color, t_out, flag

    def _light(self, c, lit, p, nrm, w0, mat, lpos, lint, kd=None, normal=None):
        """One light of the loop for the shading hits `lit` with the hits' diffuse colour `kd`
        (HW4/src/Scene.cpp:178-212 over HW2's loop: no has_diffuse / has_specular skips).  lpos,
        lint: (1, 3), or one row per hit of `lit`.  `normal` (rows as lpos): the emitter normal of
        a light sample (0 0 0: a point light), HW3/src/Scene.cpp:207-218."""
        if kd is None:
            kd = self.kd[mat]
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
        kdi = kd[lit] * lint
        ksi = self.ks[m] * lint
        if normal is not None:
            point = (normal == 0).all(axis=1)
            ic = _dot(-wi, np.broadcast_to(normal, wi.shape))
            kdi = np.where(point[:, None], kdi, kdi * ic[:, None])
            ksi = np.where(point[:, None], ksi, ksi * ic[:, None])
        dif = (kdi * cos_d[:, None]) / d2[:, None]
        hv = w0[lit] + wi
        cos_s = np.fmax(_dot(nrm[lit], _normalize(hv)), f32(0))
        pw = _pow(cos_s, self.phong[m]).astype(f32)
        spe = (ksi * pw[:, None]) / d2[:, None]
        on = lit[~occ]
        c[on] = (c[on] + dif[~occ]) + spe[~occ]


def trace(xml, o, d, depth=-1, in_medium=False, tracer=None, **scene):
    """Scene::trace_ray(Ray(o, d, in_medium), depth) of every ray on the textured scene `scene`
    (TexTracer's arguments).  Returns (colours as a zeroed Pixel holds them, first-hit t, ray
    counts, the near-boundary flags, the tracer's `seen`)."""
    tr = tracer or TexTracer(xml, **scene)
    o = np.ascontiguousarray(o, f32)
    d = np.ascontiguousarray(d, f32)
    if depth < 0:
        depth = tr.max_depth
    with np.errstate(all="ignore"):
        color, t, flag = tr.trace(o, d, np.full(len(o), bool(in_medium)), depth)
    tr.counts["primary_rays"] = len(o)
    if tracer is None:
        tr.close()
    out = f32(0) + color
    assert out.dtype == f32 and t.dtype == f32
    return out, t, dict(tr.counts), flag, set(tr.seen)


def restate_lit(xml, o, d, own, scene_lights=False, **scene):
    """Depth-0 Scene::trace_ray of rays (o, d) with each ray's own light records `own`
    (LIGHT_SAMPLE_DTYPE, shape (n, k)) after the scene's lights (or without them), on the textured
    scene `scene`: ((n, 4) {r, g, b, t or +inf}, shadow rays cast).  The terms are lit_util.restate's;
    the diffuse colour is the texture step's."""
    tr = TexTracer(xml, **scene)
    o = np.ascontiguousarray(o, f32)
    d = np.ascontiguousarray(d, f32)
    n = len(o)
    out = np.zeros((n, 4), f32)
    out[:, 3] = np.inf
    if tr.max_depth == 0:
        out[:, :3] = tr.background
    with np.errstate(all="ignore"):
        rec, shape = tr.orc.intersect_rays(o, d)
        idx = np.flatnonzero(rec[:, 7] == 1.0)
        t = rec[idx, 3]
        nrm = tr.hit_normals(o, d, rec, shape, idx)
        mat = tr.ob.mat[shape[idx]]
        p = o[idx] + d[idx] * t[:, None]
        w0 = _normalize(o[idx] - p)
        kd, rall, texel, _ = tr.texture_step(o, d, rec, shape, idx, p, "primary")
        c = np.zeros((len(idx), 3), f32)
        c[rall] = texel[rall]
        lit = np.flatnonzero(~rall)
        c[lit] = c[lit] + tr.ka[mat[lit]] * tr.ambient[None, :]
        if scene_lights:
            for j in range(len(tr.lpos)):
                tr._light(c, lit, p, nrm, w0, mat, tr.lpos[j][None, :], tr.lint[j][None, :], kd)
        for j in range(own.shape[1]):
            L = own[idx, j]
            a = lit[np.isfinite(L["position"][lit]).all(axis=1)]
            if len(a):
                tr._light(c, a, p, nrm, w0, mat, L["position"][a], L["intensity"][a], kd,
                          L["normal"][a])
    out[idx, :3] = f32(0) + c
    out[idx, 3] = t
    shadow = tr.counts["shadow_rays"]
    tr.close()
    assert out.dtype == f32
    return out, shadow


# ---------------------------------------------------------------- the test scene
def mixed_spec():
    """tx_mixed, depth 3: a mirror and a glass icosphere (smooth, untextured), a two-triangle floor
    quad, a back wall (smooth), a loose triangle whose material is a mirror, a sphere, two lights.
    Cameras: 33 x 31, 17 x 9 (partial tiles), and 17 x 9 with NumSamples 4."""
    from scenes import G
    v0, f0 = su.icosphere((-1.15, 0.0, 0.0), 1.0)
    v1, f1 = su.icosphere((1.15, 0.0, 0.1), 1.0)
    floor = [(-4.0, -1.2, -4.0), (4.0, -1.2, -4.0), (4.0, -1.2, 4.0), (-4.0, -1.2, 4.0)]
    wall = [(-5.0, -1.2, -3.0), (5.0, -1.2, -3.0), (5.0, 4.0, -3.0), (-5.0, 4.0, -3.0)]
    loose = [(-2.75, 0.75, 0.5), (-1.5, 1.0, 0.5), (-2.25, 2.0, 0.25)]
    centre = [(0.25, 1.75, -1.0)]
    verts = v0 + v1 + floor + wall + loose + centre
    text = lambda faces, base: "\n".join(" ".join(str(i + base + 1) for i in f) for f in faces)  # noqa: E731
    b2 = len(v0) + len(v1)
    quad = lambda b: f"{b + 1} {b + 3} {b + 2}\n{b + 1} {b + 4} {b + 3}"  # noqa: E731
    facing = lambda b: f"{b + 1} {b + 2} {b + 3}\n{b + 1} {b + 3} {b + 4}"  # noqa: E731
    view = ((0.2, 1.0, 4.5), (0, -0.2, -1), (0, 1, 0), (-0.7, 0.7, -0.66, 0.66), 1)
    cams = [G.Camera(*view, 33, 31, "tx0.png"), G.Camera(*view, 17, 9, "tx1.png"),
            G.Camera(*view, 17, 9, "tx2.png", num_samples=4)]
    return G.SceneSpec(
        cameras=cams, ambient=(15, 15, 15), background=(10, 20, 40), max_depth=3,
        lights=[((0.0, 5.0, 4.0), (900, 900, 900)), ((-4.0, 3.0, 1.0), (500, 400, 300))],
        materials=[G.Material((1, 1, 1), (0.2, 0.2, 0.3), (0.6, 0.6, 0.6), mirror=(0.7, 0.7, 0.7),
                              phong=20),
                   G.Material((1, 1, 1), (0.05, 0.05, 0.05), (0.4, 0.4, 0.4), phong=30,
                              transparency=(0.9, 0.8, 0.7), refraction_index=1.5),
                   G.Material((1, 1, 1), (0.6, 0.7, 0.5), (0.1, 0.1, 0.1), phong=2),
                   G.Material((1, 1, 1), (0.5, 0.4, 0.7), (0.2, 0.2, 0.2), phong=4),
                   G.Material((1, 1, 1), (0.3, 0.3, 0.3), (0.5, 0.5, 0.5), mirror=(0.5, 0.5, 0.5),
                              phong=8),
                   G.Material((1, 1, 1), (0.7, 0.6, 0.5), (0.3, 0.3, 0.3), phong=6)],
        vertex_text=su._verts(verts),
        meshes=[(1, text(f0, 0)), (2, text(f1, len(v0))), (3, quad(b2)), (4, facing(b2 + 4))],
        triangles=[(5, (b2 + 9, b2 + 10, b2 + 11))], spheres=[(6, b2 + 12, 0.75)])


MIXED_SMOOTH = (0, 1, 3)


def mixed_scene(directory):
    """tx_mixed: (xml, desc, the TexTracer / Scene.create keyword arguments)."""
    xml = su.write_spec(mixed_spec(), directory, "tx_mixed", MIXED_SMOOTH)
    desc = desc_xml.Desc(xml)
    nv = desc.d.num_vertices
    uv = np.zeros((nv, 2), f32)
    b2 = nv - 12
    uv[b2:b2 + 4] = [(0.0, 0.0), (2.5, 0.0), (2.5, 2.5), (0.0, 2.5)]          # floor: repeat
    uv[b2 + 4:b2 + 8] = [(-0.125, 1.125), (1.125, 1.125), (1.125, -0.125), (-0.125, -0.125)]  # wall: clamp
    uv[b2 + 8:b2 + 11] = [(0.0, 0.0), (1.0, 0.0), (0.5, 1.0)]
    textures = [random_texture(3, 2, 11, interpolation=NEAREST, decal=REPLACE_KD, appearance=REPEAT),
                random_texture(4, 4, 12, interpolation=BILINEAR, decal=BLEND_KD, appearance=CLAMP),
                random_texture(2, 3, 13, interpolation=BILINEAR, decal=REPLACE_ALL, appearance=CLAMP),
                random_texture(5, 7, 14, interpolation=BILINEAR, decal=REPLACE_KD, appearance=REPEAT,
                               normalizer=200.0)]
    scene = dict(textures=textures, mesh_texture=[-1, -1, 0, 1], triangle_texture=[2],
                 sphere_texture=[3], uv=uv, smooth=MIXED_SMOOTH)
    return xml, desc, scene


def create_kwargs(desc, scene):
    """Scene.create's keyword arguments for a TexTracer scene."""
    flags = su.mesh_flags(desc, scene.get("smooth", ()))
    return dict(mesh_smooth=flags if flags.any() else None, vertex_uv=scene.get("uv"),
                textures=scene["textures"], mesh_texture=scene.get("mesh_texture"),
                triangle_texture=scene.get("triangle_texture"),
                sphere_texture=scene.get("sphere_texture"))


_REFERENCE = {}


def reference(directory, depth=-1, in_medium=False, camera=0):
    """tx_mixed's camera rays (rq_util.Batch) and `trace` of them, computed once per (depth,
    medium, camera) and shared: (batch, rgb, t, counts, near flags, seen)."""
    key = (directory, depth, in_medium, camera)
    if key not in _REFERENCE:
        xml, _, scene = mixed_scene(directory)
        b = rq_util.oracle_batch(xml, cameras=[camera])
        rgb, t, counts, flag, seen = trace(xml, b.o, b.d, depth, in_medium, **scene)
        for a in (rgb, t, b.o, b.d, flag):
            a.setflags(write=False)
        _REFERENCE[key] = (b, rgb, t, counts, flag, seen)
    return _REFERENCE[key]


# ---------------------------------------------------------------- inputs the test files share
import itertools  # noqa: E402

SIZES = [(1, 1), (2, 2), (3, 2), (2, 3), (4, 4), (5, 7)]  # (w, h)
MODES = list(itertools.product((NEAREST, BILINEAR), (REPEAT, CLAMP)))


def grid_queries(w, h):
    us, vs = edge_coordinates(w), edge_coordinates(h)
    u, v = np.meshgrid(us, vs, indexing="ij")
    return u.reshape(-1), v.reshape(-1)


def lit_records(b):
    """One emitter record per ray above the floor (the GPU test's records)."""
    import ceng795_amd
    import lit_util
    rng = np.random.default_rng(5)
    n = len(b)
    own = np.zeros((n, 1), ceng795_amd.LIGHT_SAMPLE_DTYPE)
    own["position"][:, 0] = np.stack([lit_util.eighths(rng, -3, 3, n), lit_util.eighths(rng, 2, 4, n),
                                      lit_util.eighths(rng, 0, 3, n)], axis=1)
    own["intensity"][:, 0] = (300, 400, 500)
    own["normal"][:, 0] = (0, -1, 0)
    return own


def replace_all_rays(desc, n=200):
    """n rays from one point to seeded points inside the loose triangle."""
    v = desc.verts.reshape(-1, 3)
    a, b, c = (v[i] for i in desc.arrays["triangle_indices"][:3])
    rng = np.random.default_rng(9)
    w = rng.dirichlet((1, 1, 1), n).astype(np.float32) * np.float32(0.9) + np.float32(0.1 / 3)
    target = w[:, :1] * a + w[:, 1:2] * b + w[:, 2:] * c
    o = np.broadcast_to(np.array([0.2, 1.0, 4.5], np.float32), (n, 3)).copy()
    d = (target - o).astype(np.float32)
    return o, np.ascontiguousarray(d / np.sqrt((d * d).sum(axis=1, dtype=np.float32))[:, None])


# ---------------------------------------------------------------- scene files
_INTERPOLATION = {NEAREST: "nearest", BILINEAR: "bilinear"}
_DECAL = {REPLACE_KD: "replace_kd", BLEND_KD: "blend_kd", REPLACE_ALL: "replace_all"}
_APPEARANCE = {REPEAT: "repeat", CLAMP: "clamp"}


def textured_xml(directory, name="tx_mixed_file", defaults=(), change=None):
    """tx_mixed as a scene file with HW4's texture tags: <TexCoordData>, the root <Textures> block
    and a 1-based <Texture> child per textured object.  `defaults`: the textures whose mode tags
    and <Normalizer> are left out although they hold the reference's defaults.  `change`: a
    function of the text, for the refused variants.  Returns (path, the images by name, scene)."""
    import os
    xml, desc, scene = mixed_scene(directory)
    text = open(xml).read()
    uv = scene["uv"]
    pairs = "\n".join(f"{float(a)!r} {float(b)!r}" for a, b in uv)
    block = ["  <Textures>"]
    images = {}
    for k, tex in enumerate(scene["textures"]):
        images[f"tex{k}.png"] = tex["rgb8"]
        block.append(f'    <Texture id="{k + 1}">')
        block.append(f"      <ImageName>tex{k}.png</ImageName>")
        if k not in defaults:
            block.append(f"      <Interpolation>{_INTERPOLATION[tex['interpolation']]}</Interpolation>")
            block.append(f"      <DecalMode>{_DECAL[tex['decal']]}</DecalMode>")
            block.append(f"      <Appearance>{_APPEARANCE[tex['appearance']]}</Appearance>")
            block.append(f"      <Normalizer>{float(tex['normalizer'])!r}</Normalizer>")
        block.append("    </Texture>")
    block.append("  </Textures>")
    text = text.replace("  <Objects>", f"  <TexCoordData>\n{pairs}\n  </TexCoordData>\n" +
                        "\n".join(block) + "\n  <Objects>")
    for kind, ids in (("Mesh", scene["mesh_texture"]), ("Triangle", scene["triangle_texture"]),
                      ("Sphere", scene["sphere_texture"])):
        for k, tid in enumerate(ids):
            if tid < 0:
                continue
            at = text.index(f'<{kind} id="{k + 1}"')
            end = text.index("</Material>", at) + len("</Material>")
            text = text[:end] + f"\n      <Texture>{tid + 1}</Texture>" + text[end:]
    if change:
        text = change(text)
    path = os.path.join(directory, name + ".xml")
    tmp = path + f".{os.getpid()}.tmp"
    with open(tmp, "w") as f:
        f.write(text)
    os.replace(tmp, path)
    return path, images, scene
