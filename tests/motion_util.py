"""Reference for scenes with motion, composed from instance_util's composite.

What HW3 adds for motion blur, restated in numpy fp32 with every product and sum rounded once:

    per-ray matrix     Translation(time * velocity) * M by Matrix4x4::operator* (every entry from 0
                       through its four products, the ones with 0 and 1 included), then
                       invert_matrix — both vectorised over the rays (Mesh.h:75-92)
    boxes              expanded by +-velocity after apply_transform (Mesh.h:104-110, Sphere.h:30-36)
    spheres            a transformed or moving sphere is its own one-sphere oracle scene met with
                       the local ray; normal through the inverse's transpose (Sphere.h:76-154)

A MotionComposite answers for rays at a time: `set_time(scalar or (n,))`, then the base class's
intersect / occluded.  instance_util.trace threads no time through its secondary rays, so a ray
tree is restated once per distinct time with a scalar time (trace_at).  Checked against goldens
from HW3's compiled code, every ray and every field (tests/test_ref_hw34_host.py)."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import instance_util as iu
from instance_util import F, INF


# ------------------------------------------------------------------ batched matrices
_P, _N = 1, -1
_COFACTORS = {
    0: [(_P, 5, 10, 15), (_N, 5, 11, 14), (_N, 9, 6, 15), (_P, 9, 7, 14), (_P, 13, 6, 11), (_N, 13, 7, 10)],
    4: [(_N, 4, 10, 15), (_P, 4, 11, 14), (_P, 8, 6, 15), (_N, 8, 7, 14), (_N, 12, 6, 11), (_P, 12, 7, 10)],
    8: [(_P, 4, 9, 15), (_N, 4, 11, 13), (_N, 8, 5, 15), (_P, 8, 7, 13), (_P, 12, 5, 11), (_N, 12, 7, 9)],
    12: [(_N, 4, 9, 14), (_P, 4, 10, 13), (_P, 8, 5, 14), (_N, 8, 6, 13), (_N, 12, 5, 10), (_P, 12, 6, 9)],
    1: [(_N, 1, 10, 15), (_P, 1, 11, 14), (_P, 9, 2, 15), (_N, 9, 3, 14), (_N, 13, 2, 11), (_P, 13, 3, 10)],
    5: [(_P, 0, 10, 15), (_N, 0, 11, 14), (_N, 8, 2, 15), (_P, 8, 3, 14), (_P, 12, 2, 11), (_N, 12, 3, 10)],
    9: [(_N, 0, 9, 15), (_P, 0, 11, 13), (_P, 8, 1, 15), (_N, 8, 3, 13), (_N, 12, 1, 11), (_P, 12, 3, 9)],
    13: [(_P, 0, 9, 14), (_N, 0, 10, 13), (_N, 8, 1, 14), (_P, 8, 2, 13), (_P, 12, 1, 10), (_N, 12, 2, 9)],
    2: [(_P, 1, 6, 15), (_N, 1, 7, 14), (_N, 5, 2, 15), (_P, 5, 3, 14), (_P, 13, 2, 7), (_N, 13, 3, 6)],
    6: [(_N, 0, 6, 15), (_P, 0, 7, 14), (_P, 4, 2, 15), (_N, 4, 3, 14), (_N, 12, 2, 7), (_P, 12, 3, 6)],
    10: [(_P, 0, 5, 15), (_N, 0, 7, 13), (_N, 4, 1, 15), (_P, 4, 3, 13), (_P, 12, 1, 7), (_N, 12, 3, 5)],
    14: [(_N, 0, 5, 14), (_P, 0, 6, 13), (_P, 4, 1, 14), (_N, 4, 2, 13), (_N, 12, 1, 6), (_P, 12, 2, 5)],
    3: [(_N, 1, 6, 11), (_P, 1, 7, 10), (_P, 5, 2, 11), (_N, 5, 3, 10), (_N, 9, 2, 7), (_P, 9, 3, 6)],
    7: [(_P, 0, 6, 11), (_N, 0, 7, 10), (_N, 4, 2, 11), (_P, 4, 3, 10), (_P, 8, 2, 7), (_N, 8, 3, 6)],
    11: [(_N, 0, 5, 11), (_P, 0, 7, 9), (_P, 4, 1, 11), (_N, 4, 3, 9), (_N, 8, 1, 7), (_P, 8, 3, 5)],
    15: [(_P, 0, 5, 10), (_N, 0, 6, 9), (_N, 4, 1, 10), (_P, 4, 2, 9), (_P, 8, 1, 6), (_N, 8, 2, 5)],
}


def invert_batch(mats):
    """Matrix4x4::invert_matrix of every matrix of (n, 16) at once: (inverse (n, 16), ok (n,)).
    Where the determinant is 0 the inverse is NaN and ok False."""
    m = np.ascontiguousarray(mats, F).reshape(-1, 16)
    c = np.zeros_like(m)
    with np.errstate(all="ignore"):
        for e, terms in _COFACTORS.items():
            acc = None
            for sign, i, j, k in terms:
                first = -m[:, i] if (acc is None and sign < 0) else m[:, i]
                p = ((first * m[:, j]).astype(F) * m[:, k]).astype(F)
                if acc is None:
                    acc = p
                elif sign > 0:
                    acc = (acc + p).astype(F)
                else:
                    acc = (acc - p).astype(F)
            c[:, e] = acc
        det = (m[:, 0] * c[:, 0]).astype(F)
        for a, b in ((1, 4), (2, 8), (3, 12)):
            det = (det + (m[:, a] * c[:, b]).astype(F)).astype(F)
        ok = det != 0
        r = (F(1.0) / det).astype(F)
        inv = (c * r[:, None]).astype(F)
    inv[~ok] = np.nan
    return inv, ok


def motion_matrix(fwd, vel, tau):
    """T(tau * vel) * fwd per ray, (n, 16): Matrix4x4::operator* with T written out."""
    M = np.asarray(fwd, F).reshape(4, 4)
    tau = np.asarray(tau, F).reshape(-1)
    n = len(tau)
    T = np.zeros((n, 4, 4), F)
    for i in range(4):
        T[:, i, i] = 1
    with np.errstate(all="ignore"):
        for i in range(3):
            T[:, i, 3] = (tau * F(vel[i])).astype(F)
        out = np.zeros((n, 4, 4), F)
        for i in range(4):
            for j in range(4):
                acc = np.zeros(n, F)
                for k in range(4):
                    acc = (acc + (T[:, i, k] * M[k, j]).astype(F)).astype(F)
                out[:, i, j] = acc
    return out.reshape(n, 16)


def motion_inverse(fwd, vel, tau):
    """Rows 0..2 of the per-ray inverse, (n, 12) (NaN where det == 0), and ok (n,)."""
    inv, ok = invert_batch(motion_matrix(fwd, vel, tau))
    return inv[:, :12].copy(), ok


def multiply_batch(inv, v, is_vector=False):
    """Matrix4x4::multiply with one matrix per row: inv (n, >= 12) row-major, v (n, 3)."""
    e = np.asarray(inv, F).reshape(len(v), -1)
    v = np.asarray(v, F)
    out = np.zeros_like(v)
    with np.errstate(all="ignore"):
        for i in range(3):
            r = np.zeros(len(v), F) if is_vector else e[:, 4 * i + 3].copy()
            for j in range(3):
                r = (r + (e[:, 4 * i + j] * v[:, j]).astype(F)).astype(F)
            out[:, i] = r
    return out


def normal_batch(inv, nrm):
    """(inverse)^T.multiply(n, true).normalize() with one matrix per row."""
    e = np.asarray(inv, F).reshape(len(nrm), -1)
    out = np.zeros_like(nrm)
    with np.errstate(all="ignore"):
        for i in range(3):
            r = np.zeros(len(nrm), F)
            for j in range(3):
                r = (r + (e[:, 4 * j + i] * nrm[:, j]).astype(F)).astype(F)
            out[:, i] = r
        ln = np.sqrt(((out[:, 0] * out[:, 0]).astype(F) + (out[:, 1] * out[:, 1]).astype(F)).astype(F)
                     + (out[:, 2] * out[:, 2]).astype(F)).astype(F)
        return (out / ln[:, None]).astype(F)


def expand_box(box, v):
    """Bounding_box::expand by (min + v, max + v), then by (min - v, max - v)."""
    box = np.asarray(box, F)
    v = np.asarray(v, F)
    lo, hi = box[:3], box[3:]
    nlo = np.fmin(np.fmin(lo, (lo + v).astype(F)), (lo - v).astype(F))
    nhi = np.fmax(np.fmax(hi, (hi + v).astype(F)), (hi - v).astype(F))
    return np.concatenate([nlo, nhi]).astype(F)


def _moves(v):
    return v is not None and bool((np.asarray(v, F) != 0).any())


# ------------------------------------------------------------------ scenes
@dataclass
class MotionSpec(iu.InstSpec):
    """An InstSpec with a velocity per instance and, per sphere, a matrix and a velocity (None:
    zero / the identity)."""
    velocity: list = field(default_factory=list)
    sphere_xf: list = field(default_factory=list)
    sphere_vel: list = field(default_factory=list)

    def motion_arrays(self):
        ni, ns = len(self.instances), len(self.spheres)
        vel = np.array([v if v is not None else (0, 0, 0) for v in (self.velocity or [None] * ni)], F).reshape(ni, 3)
        xf = np.array([x if x is not None else np.eye(4) for x in (self.sphere_xf or [None] * ns)], F).reshape(ns, 4, 4)
        sv = np.array([v if v is not None else (0, 0, 0) for v in (self.sphere_vel or [None] * ns)], F).reshape(ns, 3)
        return vel, xf, sv

    def create(self, desc, device=0):
        import ceng795_amd
        vel, xf, sv = self.motion_arrays()
        kw = {}
        if self.instances:
            mesh, mat, m = self.arrays()
            kw = dict(instance_mesh=mesh, instance_material=mat, instance_transform=m)
        return ceng795_amd.Scene.create(desc, device=device, instance_velocity=vel if self.instances else None,
                                        sphere_transform=xf if self.spheres else None,
                                        sphere_velocity=sv if self.spheres else None, **kw)


class MotionComposite(iu.Composite):
    """The reference for one written MotionSpec.  Rays are answered at the time last set."""

    def __init__(self, spec: MotionSpec):
        super().__init__(spec)
        self.vel, self.sphere_xf, self.sphere_vel = spec.motion_arrays()
        V = np.array(spec.vertices, F)
        boxes = []
        for i, (mesh, _, mat) in enumerate(spec.instances):
            if _moves(self.vel[i]):
                self.inst_box[i] = expand_box(self.inst_box[i], self.vel[i])
            boxes.append(self.inst_box[i])
        for _, t in spec.triangles:
            pts = V[list(t)]
            boxes.append(np.concatenate([pts.min(0), pts.max(0)]).astype(F))
        self.sphere_inverse, self.sphere_box = [], []
        for k, (_, c, r) in enumerate(spec.spheres):
            box = np.concatenate([(V[c] - F(r)).astype(F), (V[c] + F(r)).astype(F)])
            m = self.sphere_xf[k]
            placed = not np.array_equal(m, np.eye(4, dtype=F))
            self.sphere_inverse.append(iu.invert_matrix(m) if placed else np.eye(4, dtype=F))
            if placed:
                box = iu.apply_transform(box, m)
            if _moves(self.sphere_vel[k]):
                box = expand_box(box, self.sphere_vel[k])
            self.sphere_box.append(box)
            boxes.append(box)
        self.boxes = boxes
        self.order, self.paths = iu.top_level_tree(boxes)
        self.top_of = {obj: pos for pos, obj in enumerate(self.order)}
        self._time = F(0)

    # -- the time of the rays of the next intersect / occluded call
    def set_time(self, time):
        self._time = np.asarray(time, F)
        return self

    def _tau(self, n):
        return np.broadcast_to(self._time, (n,)).astype(F)

    def sphere_special(self, k):
        return _moves(self.sphere_vel[k]) or not np.array_equal(self.sphere_xf[k], np.eye(4, dtype=F))

    def instance_inverse(self, i, n):
        """(n, 16-or-12) per-ray inverse of instance i at the set time."""
        if _moves(self.vel[i]):
            return motion_inverse(self.spec.instances[i][2], self.vel[i], self._tau(n))[0]
        return np.broadcast_to(np.asarray(self.inverse[i], F).reshape(16)[:12], (n, 12))

    def local_rays(self, i, o, d):
        inv = self.instance_inverse(i, len(o))
        return multiply_batch(inv, o), multiply_batch(inv, d, True)

    def object_hits(self, obj, o, d):
        n = len(o)
        spec = self.spec
        ni = len(spec.instances)
        if obj < ni:
            mesh, material, _ = spec.instances[obj]
            inv = self.instance_inverse(obj, n)
            lo, ld = multiply_batch(inv, o), multiply_batch(inv, d, True)
            go = iu.slab_accept(self.inst_box[obj], o, d) & iu.ray_ok(lo, ld)
            rec, shape = self.mesh_orc[mesh].intersect_rays(np.where(go[:, None], lo, F(0)),
                                                            np.where(go[:, None], ld, F(1)))
            hit = go & (rec[:, 7] == 1.0)
            nrm = normal_batch(inv, rec[:, 4:7])
            face = np.where(hit, shape, 0)
            return (hit, rec[:, 3], self.face_base[mesh] + face, np.full(n, material, np.int32),
                    self.leaf_base[mesh] + self.leaf_of_face[mesh][face], np.full(n, obj, np.int32), nrm)
        k = obj - ni - len(spec.triangles)
        if k < 0 or not self.sphere_special(k):
            return super().object_hits(obj, o, d)
        if _moves(self.sphere_vel[k]):
            inv = motion_inverse(self.sphere_xf[k], self.sphere_vel[k], self._tau(n))[0]
        else:
            inv = np.broadcast_to(np.asarray(self.sphere_inverse[k], F).reshape(16)[:12], (n, 12))
        lo, ld = multiply_batch(inv, o), multiply_batch(inv, d, True)
        go = iu.ray_ok(lo, ld)
        rec, _ = self.loose_orc[obj - ni].intersect_rays(np.where(go[:, None], lo, F(0)),
                                                         np.where(go[:, None], ld, F(1)))
        hit = go & (rec[:, 7] == 1.0)
        nrm = normal_batch(inv, rec[:, 4:7])
        lk = obj - ni
        return (hit, rec[:, 3], np.full(n, self.total_faces + lk, np.int32),
                np.full(n, spec.spheres[k][0], np.int32), np.full(n, self.mesh_leaves + lk, np.int32),
                np.full(n, -1, np.int32), nrm)

    def _masked(self, o):
        """Origins with NaN where the ray's time is not finite: an invalid ray."""
        o = np.ascontiguousarray(o, F).reshape(-1, 3).copy()
        bad = ~np.isfinite(self._tau(len(o)))
        o[bad] = np.nan
        if bad.any():
            self._time = np.where(bad, F(0), self._tau(len(o)))
        return o

    def intersect(self, o, d, time=None):
        if time is not None:
            self.set_time(time)
        return super().intersect(self._masked(o), d)

    def occluded(self, o, d, tmax, time=None):
        if time is not None:
            self.set_time(time)
        return super().occluded(self._masked(o), d, tmax)

    def winner_kind(self, ref):
        """Per ray: 'moving_instance', 'static_instance', 'moving_sphere', 'placed_sphere',
        'sphere', 'triangle' or 'miss'."""
        ni, nt = len(self.spec.instances), len(self.spec.triangles)
        out = np.full(len(ref.hit), "miss", object)
        for i in np.nonzero(ref.hit)[0]:
            obj = self.order[ref.top[i]]
            if obj < ni:
                out[i] = "moving_instance" if _moves(self.vel[obj]) else "static_instance"
            elif obj < ni + nt:
                out[i] = "triangle"
            else:
                k = obj - ni - nt
                out[i] = ("moving_sphere" if _moves(self.sphere_vel[k]) else
                          "placed_sphere" if self.sphere_special(k) else "sphere")
        return out


def trace_at(comp, o, d, time, depth=-1, in_medium=False):
    """instance_util.trace of rays with per-ray times: once per distinct time, on that time's rays,
    with a scalar time.  Returns (colour (n, 3), t (n,), summed ray counts)."""
    o = np.ascontiguousarray(o, F)
    d = np.ascontiguousarray(d, F)
    time = np.broadcast_to(np.asarray(time, F), (len(o),))
    color = np.zeros((len(o), 3), F)
    t = np.full(len(o), INF, F)
    counts = {}
    for tau in np.unique(time):
        sel = time == tau
        comp.set_time(F(tau))
        c, tt, cnt = iu.trace(comp, o[sel], d[sel], depth, in_medium)
        color[sel], t[sel] = c, tt
        for k, v in cnt.items():
            counts[k] = counts.get(k, 0) + v
    return color, t, counts


# ------------------------------------------------------------------ test geometry
VEL_CHAIN = (0.8, -0.5, 0.3)
VEL_LIFT = (-0.4, 0.3, -0.0)
VEL_SPHERE = (0.6, 0.9, -0.4)


def _with_spheres(spec_fn):
    """scene_three's geometry with two more sphere centres."""
    base = spec_fn()
    verts = list(base.vertices) + [(-0.8, 2.4, 0.6), (1.2, -2.6, 0.9)]
    return base, verts, len(base.vertices), len(base.vertices) + 1


def scene_main(materials=None, max_depth=0, lights=None, camera=None):
    """Scene "three" with motion: the composed instance and the one-face instance move, the identity
    and the mirrored one stand; the plain sphere, a moving sphere under the identity and a static
    sphere under a non-uniform scaling; the loose triangle."""
    base, verts, c1, c2 = _with_spheres(iu.scene_three)
    placed = iu.matmul(iu.translation(0.4, -0.3, 0.2), iu.matmul(iu.rotation_z(20.0), iu.scaling(1.4, 0.6, 0.8)))
    spec = MotionSpec(verts, base.meshes, base.instances, triangles=base.triangles,
                      spheres=base.spheres + [(1, c1, 0.5), (0, c2, 0.45)],
                      materials=materials or base.materials,
                      velocity=[None, VEL_CHAIN, None, VEL_LIFT],
                      sphere_xf=[None, None, placed], sphere_vel=[None, VEL_SPHERE, None])
    spec.max_depth = max_depth
    if lights:
        spec.lights = lights
    if camera:
        spec.camera = camera
    return spec


def scene_still():
    """scene_main's objects with every velocity zero and every sphere matrix the identity."""
    spec = scene_main()
    spec.velocity, spec.sphere_xf, spec.sphere_vel = [], [], []
    return spec


def scene_lone_sphere():
    """One moving sphere under a non-uniform scaling: its own rule, negative roots included."""
    base, verts, c1, c2 = _with_spheres(iu.scene_three)
    return MotionSpec(verts, [], [], spheres=[(1, c1, 0.7)], materials=base.materials,
                      sphere_xf=[iu.scaling(1.5, 0.7, 1.1)], sphere_vel=[VEL_SPHERE])


def scene_lone_instance():
    base = iu.scene_single()
    return MotionSpec(base.vertices, base.meshes, base.instances, materials=base.materials,
                      velocity=[VEL_CHAIN])


def scene_scaled():
    """instance_util's 1e7 / 1e-3 scalings (the skipped-axis cases of §4.16), each instance
    moving along an axis its scaling leaves alone."""
    base = iu.scene_scaled()
    return MotionSpec(base.vertices, base.meshes, base.instances, triangles=base.triangles,
                      materials=base.materials,
                      velocity=[(0.0, 0.5, 0.0), (0.5, 0.0, 0.0), (0.0, 0.0, -0.5)])


def scene_det_zero():
    """An instance whose per-ray determinant is exactly 0 at some times though its matrix is
    invertible.  det(T(d) M) = det(M) in exact arithmetic, so only rounding gets there: M is the
    identity with the bottom row (1, 0, 0, 1) — multiply() never reads that row, so at tau = 0
    the instance stands where the identity puts it — and the velocity is (2^25, 0, 0).  Then
    A[0][0] = fl(1 + a), A[0][3] = a, A[3][0] = A[3][3] = 1 with a = tau 2^25, and the computed
    determinant is fl(fl(1 + a) - a): 1 while 1 + a is exact (tau <= 2^-2), 0 from tau = 2^-1 on
    (DET_ZERO_TIMES / DET_ONE_TIMES).  Beside it a loose triangle, which such rays still hit."""
    base = iu.scene_single()
    verts, faces, one, tri, centre = iu._geometry()
    m = np.eye(4, dtype=F)
    m[3, 0] = 1
    return MotionSpec(verts, [faces], [(0, 1, m)], triangles=[(0, tri)],
                      materials=base.materials, velocity=[(float(2 ** 25), 0.0, 0.0)])


DET_ZERO_TIMES = np.array([0.5, 1.0, 0.75], F)
DET_ONE_TIMES = np.array([0.0, 2.0 ** -10, 2.0 ** -20], F)


def scene_shiny(samples=None, width=33, height=31):
    """scene_main with a moving mirror instance and a moving glass sphere, MaxRecursionDepth 3, two
    lights (instance_util.scene_shiny's materials and camera)."""
    shiny = iu.scene_shiny(samples, width, height)
    spec = scene_main(materials=shiny.materials, max_depth=3, lights=shiny.lights, camera=shiny.camera)
    spec.instances = [(m, {1: 3}.get(i, mat), x) for i, (m, mat, x) in enumerate(spec.instances)]
    spec.spheres = [(4 if k == 1 else m, c, r) for k, (m, c, r) in enumerate(spec.spheres)]
    return spec


SCENES = {"main": scene_main, "still": scene_still, "lone_sphere": scene_lone_sphere,
          "lone_instance": scene_lone_instance, "scaled": scene_scaled, "det_zero": scene_det_zero,
          "shiny": scene_shiny, "shiny_msaa": lambda: scene_shiny(samples=4, width=17, height=9)}


def written(name, directory):
    return SCENES[name]().write(directory, "motion_" + name)


def main_batch(seed=5):
    """(o, d, time) at scene_main: rays from a shell around the scene toward it with times in
    [0, 1); rays aimed at where the loose triangle, the plain and the placed sphere stand and at
    where the moving instance and the moving sphere are at the ray's own time; and rays at times
    6 and -5 aimed at where the moving instance is then — far outside its box."""
    rng = np.random.default_rng(seed)
    parts = []

    def aimed(n, centre, spread, tau, vel=(0, 0, 0)):
        tau = np.broadcast_to(np.asarray(tau, F), (n,)).astype(F)
        o = (rng.normal(size=(n, 3)) * 4).astype(F)
        target = np.asarray(centre) + tau[:, None].astype(np.float64) * np.asarray(vel) + \
            rng.uniform(-spread, spread, size=(n, 3))
        parts.append((o, (target.astype(F) - o).astype(F), tau))

    o, d = iu.random_rays(250, seed + 1)
    parts.append((o, d, rng.random(250).astype(F)))
    aimed(60, (-2.5, -1.67, -1.0), 0.3, rng.random(60))
    aimed(150, (2.5, 1.0, -0.4), 0.7, rng.random(150), VEL_CHAIN)
    aimed(100, (-0.8, 2.4, 0.6), 0.4, rng.random(100), VEL_SPHERE)
    placed = iu.matmul(iu.translation(0.4, -0.3, 0.2), iu.matmul(iu.rotation_z(20.0), iu.scaling(1.4, 0.6, 0.8)))
    aimed(60, (placed.astype(np.float64) @ np.array([1.2, -2.6, 0.9, 1.0]))[:3], 0.3, rng.random(60))
    aimed(40, (2.5, -1.5, -0.5), 0.4, rng.random(40))
    aimed(40, (2.5, 1.0, -0.4), 0.5, 6.0, VEL_CHAIN)
    aimed(40, (2.5, 1.0, -0.4), 0.5, -5.0, VEL_CHAIN)
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def missed_at_the_box(comp, o, d, time):
    """Rays that some moving instance's mesh would answer with 0 < t < inf at the ray's time but
    for the instance box (which does not move): the object is outside its box then."""
    comp.set_time(time)
    out = np.zeros(len(o), bool)
    for i, (mesh, _, _) in enumerate(comp.spec.instances):
        if not _moves(comp.vel[i]):
            continue
        lo, ld = comp.local_rays(i, o, d)
        ok = iu.ray_ok(lo, ld) & iu.ray_ok(o, d)
        rec, _ = comp.mesh_orc[mesh].intersect_rays(np.where(ok[:, None], lo, F(0)), np.where(ok[:, None], ld, F(1)))
        out |= ok & (rec[:, 7] == 1.0) & (rec[:, 3] > 0) & (rec[:, 3] < INF) & ~iu.slab_accept(comp.inst_box[i], o, d)
    return out


SPECIAL_TIMES = np.array([0.0, 1.0, -1.0, 1.5, -0.0], F)
