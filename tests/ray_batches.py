"""Seeded ray batches no camera can generate, for the ray- and radiance-query tests: scattered
origins (inside the boxes, on surfaces, behind the geometry, far outside the shared-reciprocal
range), unnormalised directions over 72 binades, directions at the slab test's 1e-6 skip
threshold.  numpy only, fp32 throughout, no transcendental functions (only + - * / sqrt, which
IEEE 754 fixes), so a batch is the same bytes on every machine: tests/golden/golden_rays.npz
holds rays of these batches with the reference's own answers.

A batch knows nothing of the GPU.  What the generator needs from the scene — the root box, the
lights, the shadow epsilon, and the oracle's hits of camera 0 (the surface points rays start
on) — is a SceneInfo, built once per scene by scene_info(xml).

Each family's *mix conditions* (check_mix) are asserted from the oracle alone: they name the
branch of the kernels the family is there to force both ways, so a batch cannot be vacuous."""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass

import numpy as np

F = np.float32
INF = F(np.inf)
EPS_SKIP = F(1e-6)  # HW2/bounding_box.cpp:21
# 2^45 alone leaves too few of hf_small's small triangles outside tri_quotients' |det| <= 2^40
# (56 rays): hence 2^52 and 2^60.
SCALES = np.array([2.0 ** -12, 2.0 ** -3, 0.37, 1.0, 3.7, 2.0 ** 10, 2.0 ** 25, 2.0 ** 45,
                   2.0 ** 52, 2.0 ** 60], F)
THRESHOLD_VALUES = np.array([0.0, np.nextafter(F(1e-6), F(0)), F(1e-6), np.nextafter(F(1e-6), F(1))],
                            F)
OTHER_VALUES = np.array([1.0, 3e-6, 1e-5], F)  # (the O(1) one is scaled by a random 0.3 .. 1)
SMALL_COORDS = np.array([2.0 ** -27, -2.0 ** -27, 1e-30, -1e-30, 1e-40, -0.0], F)
LARGE_COORDS = np.array([2.0 ** 49, -2.0 ** 49, 2.0 ** 60, -2.0 ** 60], F)
FAMILIES = ("interior", "surface", "scaled", "threshold", "range")

N_INTERIOR = 8192
N_SURFACE = 1024       # points of (a) and of (b)
N_SHADOW = 4096        # rays of (c), as whole points x targets
N_SCALED_INTERIOR = 7168
N_THRESHOLD = 6144
N_RANGE = 8192


@dataclass
class SceneInfo:
    name: str
    lo: np.ndarray        # root box
    hi: np.ndarray
    lights: np.ndarray    # (L, 3)
    eps: np.float32       # ShadowRayEpsilon
    p: np.ndarray         # (k, 3) camera 0's hit points o + d t, in ray order
    n: np.ndarray         # (k, 3) their Hit_data::normal
    shape: np.ndarray     # (k,) the primitive each lies on (object-list index)
    tri: np.ndarray       # (num objects, 3, 3) triangle vertices; NaN rows for spheres
    quot_ok: bool         # the library's scene_quot_ok: every triangle's v0 passes quot_coord


@dataclass
class Batch:
    name: str
    o: np.ndarray                  # (n, 3) float32
    d: np.ndarray                  # (n, 3) float32
    tmax: np.ndarray | None        # (n,) float32, NaN where the test is to cycle it (tmax_cycle)
    part: np.ndarray               # (n,) uint8 sub-family code (PARTS)
    aux: np.ndarray                # (n,) int32: surface: start shape; scaled: scale index;
                                   # threshold: the replaced axis a, + 4 where the origin lies
                                   # outside the root box's slab on that axis

    def __len__(self):
        return len(self.o)


PARTS = {"interior": 0, "surface_a": 1, "surface_b": 2, "surface_c": 3, "scaled_interior": 4,
         "scaled_surface": 5, "threshold": 6, "range_plain": 7, "range_small": 8, "range_large": 9}


# ---------------------------------------------------------------- fp32 helpers
def dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def length(a):
    return np.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2])


def normalize(a):
    return a / length(a)[:, None]


def seeded(name: str, family: str):
    return np.random.default_rng(zlib.crc32(f"{name}/{family}".encode()))


def uniform(rng, *shape):
    """Uniform [0, 1) as float32 (53-bit doubles rounded: the same on every platform)."""
    return rng.random(shape).astype(F)


def unit_sphere(rng, n):
    """n directions uniform on the sphere: points of the cube [-1, 1]^3 kept where
    0.01 < |p|^2 <= 1, normalised in fp32."""
    c = (uniform(rng, 3 * n + 256, 3) * F(2) - F(1)).astype(F)
    r2 = dot(c, c)
    c = c[(r2 > F(0.01)) & (r2 <= F(1))]
    assert len(c) >= n
    out = normalize(c[:n])
    assert out.dtype == F
    return out


def cosine_hemisphere(rng, normal):
    """normalize(n + u), u uniform on the unit sphere: cosine-weighted about n."""
    v = normal + unit_sphere(rng, len(normal))
    short = length(v) < F(1e-3)
    v[short] = normal[short]
    return normalize(v).astype(F)


# ---------------------------------------------------------------- the scene's side
@functools.lru_cache(maxsize=None)
def scene_info(xml: str, name: str) -> SceneInfo:
    import desc_xml
    import rq_util
    from oracle.cpu_ref import OracleScene
    desc = desc_xml.Desc(xml)
    verts = desc.verts.reshape(-1, 3)
    objects = rq_util.object_list(desc)
    tri = np.full((len(objects), 3, 3), np.nan, F)
    lo, hi = np.full(3, np.inf, F), np.full(3, -np.inf, F)
    for k, ob in enumerate(objects):
        if ob[0] == "T":
            tri[k] = verts[list(ob[1:4])]
            lo, hi = np.minimum(lo, tri[k].min(0)), np.maximum(hi, tri[k].max(0))
        else:
            c = np.array(ob[1:4], np.uint32).view(F)
            r = np.array([ob[4]], np.uint32).view(F)[0]
            lo, hi = np.minimum(lo, c - r), np.maximum(hi, c + r)
    lights = np.array([L.position[:] for L in desc.lights[:desc.d.num_lights]], F).reshape(-1, 3)
    o = OracleScene(xml)
    rec = o.primary_records(0).reshape(-1, 8)
    cam_o = np.broadcast_to(rq_util.camera_positions(xml)[0], (len(rec), 3)).astype(F)
    _, shape = o.intersect_rays(cam_o, rec[:, 0:3])
    o.close()
    hit = rec[:, 7] == 1.0
    p = (cam_o[hit] + rec[hit, 0:3] * rec[hit, 3:4]).astype(F)  # Ray::point_at: o + (t * d)
    v0 = tri[~np.isnan(tri[:, 0, 0]), 0]
    return SceneInfo(name, lo.astype(F), hi.astype(F), lights, F(desc.d.shadow_ray_epsilon), p,
                     np.ascontiguousarray(rec[hit, 4:7]), shape[hit], tri,
                     bool(quot_coord(v0).all()))


# ---------------------------------------------------------------- the families
def _batch(name, o, d, part, tmax=None, aux=None):
    o = np.ascontiguousarray(o, F)
    d = np.ascontiguousarray(d, F)
    assert o.dtype == F and d.dtype == F and o.shape == d.shape
    n = len(o)
    part = np.broadcast_to(np.asarray(part, np.uint8), (n,)).copy()
    aux = np.zeros(n, np.int32) if aux is None else np.ascontiguousarray(aux, np.int32)
    tmax = None if tmax is None else np.ascontiguousarray(tmax, F)
    return Batch(name, o, d, tmax, part, aux)


def interior(info: SceneInfo, n=N_INTERIOR) -> Batch:
    """Origins uniform in the root box scaled 1.5x about its centre.  Three directions in four
    are uniform on the sphere; the fourth (i % 4 == 3) points at one of camera 0's hit points,
    so that a scene whose geometry fills little of its box (the 99-level tree: a uniform ray
    meets a triangle once in fifty) still has its thousand hits."""
    rng = seeded(info.name, "interior")
    centre = (info.lo + info.hi) / F(2)
    half = (info.hi - info.lo) / F(2) * F(1.5)
    o = (centre + (uniform(rng, n, 3) * F(2) - F(1)) * half).astype(F)
    d = unit_sphere(rng, n)
    aimed = np.arange(n) % 4 == 3
    target = info.p[_points(info, rng, n)]
    d[aimed] = normalize((target[aimed] - o[aimed]).astype(F)).astype(F)
    return _batch("interior", o, d, PARTS["interior"])


def _points(info, rng, k):
    """k of camera 0's hit points (all of them, repeated, when it has fewer)."""
    idx = rng.permutation(len(info.p))
    idx = np.resize(idx, k)
    return idx


def shadow_targets(info: SceneInfo):
    """The scene's lights, then five stand-ins: the root box's centre, its low corner and the
    points 1/32, 1/16 and 1/8 along the diagonal from it.  A height field lit from above, one
    convex sphere or the 99-level tree shadows none or few of the points its camera sees, and
    the occluded side of surface(c) would stay empty with the lights alone (the tree: no point
    towards its light, one in five towards each of the four points near the corner)."""
    ext = info.hi - info.lo
    centre = (info.lo + info.hi) / F(2)
    near = [info.lo + ext * F(f) for f in (0.0, 1.0 / 32, 1.0 / 16, 1.0 / 8)]
    return np.concatenate([info.lights, [centre], near]).astype(F)


def surface(info: SceneInfo) -> Batch:
    rng = seeded(info.name, "surface")
    idx = _points(info, rng, N_SURFACE)
    p, nrm = info.p[idx], info.n[idx]
    wo = cosine_hemisphere(rng, nrm)
    oa = p + nrm * info.eps
    lights = shadow_targets(info)
    L = len(lights)
    k = N_SHADOW // L
    pc = np.repeat(info.p[_points(info, rng, k)], L, axis=0)
    lp = np.tile(lights, (k, 1))
    ld = lp - pc                                   # HW2/Scene.cpp:115-119, 124
    dist = length(ld)
    wi = ld / dist[:, None]
    oc = pc + wi * info.eps
    tmax_c = dist - info.eps
    nan = np.full(N_SURFACE, np.nan, F)
    b = _batch("surface", np.concatenate([oa, p, oc]), np.concatenate([wo, wo, wi]),
               np.concatenate([np.full(N_SURFACE, PARTS["surface_a"]),
                               np.full(N_SURFACE, PARTS["surface_b"]),
                               np.full(len(oc), PARTS["surface_c"])]),
               tmax=np.concatenate([nan, nan, tmax_c]),
               aux=np.concatenate([info.shape[idx], info.shape[idx], np.full(len(oc), -1)]))
    return b


def scaled(info: SceneInfo, scales=SCALES) -> Batch:
    a, s = interior(info), surface(info)
    sa = s.part == PARTS["surface_a"]
    o = np.concatenate([a.o[:N_SCALED_INTERIOR], s.o[sa]])
    d = np.concatenate([a.d[:N_SCALED_INTERIOR], s.d[sa]])
    k = np.arange(len(o)) % len(scales)
    d = (d * scales[k][:, None]).astype(F)
    return _batch("scaled", o, d,
                  np.concatenate([np.full(N_SCALED_INTERIOR, PARTS["scaled_interior"]),
                                  np.full(int(sa.sum()), PARTS["scaled_surface"])]), aux=k)


def threshold(info: SceneInfo, n=N_THRESHOLD) -> Batch:
    """d: axis a (and for every third ray a second axis b) replaced by +-THRESHOLD_VALUES, the
    others from OTHER_VALUES with random signs.  Even rays start inside the root box; odd rays
    start outside the root box's slab on axis a, on the line through one of camera 0's hit
    points where d_a != 0 (so that they can still hit), beside the box where d_a == 0."""
    rng = seeded(info.name, "threshold")
    i = np.arange(n)
    a = (i // 2) % 3
    v = (i // 6) % 8                      # value and sign of d_a
    two = (i // 48) % 3 == 2              # a second replaced axis
    b = (a + 1 + (i // 144) % 2) % 3
    sign = np.where(uniform(rng, n, 3) < F(0.5), F(-1), F(1)).astype(F)
    other = OTHER_VALUES[rng.integers(0, 3, (n, 3))]
    other = np.where(other == F(1), F(0.3) + F(0.7) * uniform(rng, n, 3), other).astype(F)
    d = (other * sign).astype(F)
    va = THRESHOLD_VALUES[v % 4] * np.where(v >= 4, F(-1), F(1)).astype(F)
    vb = THRESHOLD_VALUES[rng.integers(0, 4, n)] * sign[i, b]
    d[i, a] = va
    d[two, b[two]] = vb[two]
    ext = info.hi - info.lo
    o = (info.lo + uniform(rng, n, 3) * ext).astype(F)  # inside the root box
    out = i % 2 == 1
    q = info.p[_points(info, rng, n)]
    u = uniform(rng, n)
    da, ea = d[i, a], ext[a]
    beyond = F(0.25) * ea * (F(1) + u)                   # how far outside the slab
    # d_a != 0: o = q - d s with o_a = lo_a - beyond (d_a > 0) or hi_a + beyond (d_a < 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(da > 0, (q[i, a] - info.lo[a] + beyond) / da,
                     (q[i, a] - info.hi[a] - beyond) / da).astype(F)
    moving = out & (da != 0)
    o[moving] = (q[moving] - d[moving] * s[moving][:, None]).astype(F)
    still = out & (da == 0)
    side = np.where(u < F(0.5), info.lo[a] - beyond, info.hi[a] + beyond).astype(F)
    o[still] = q[still]
    o[still, a[still]] = side[still]
    return _batch("threshold", o, d, PARTS["threshold"], aux=a + 4 * out.astype(np.int32))


def range_(info: SceneInfo, n=N_RANGE) -> Batch:
    """interior rays; every fourth has one origin coordinate overwritten by SMALL_COORDS or
    LARGE_COORDS in turn (non-zero and below 2^-26 or above 2^48: LaneRay::quot is false for
    that lane only); with a large one d = target - o, unnormalised, the target one of camera 0's
    hit points; the small ones keep interior's direction or, in alternate rounds of the ten
    values, are aimed at such a point."""
    rng = seeded(info.name, "range")
    base = interior(info, n)
    o, d = base.o.copy(), base.d.copy()
    part = np.full(n, PARTS["range_plain"], np.uint8)
    i = np.arange(0, n, 4)
    k = (i // 4) % 10
    axis = rng.integers(0, 3, len(i))
    values = np.concatenate([SMALL_COORDS, LARGE_COORDS])
    o[i, axis] = values[k]
    large = k >= len(SMALL_COORDS)
    part[i] = np.where(large, PARTS["range_large"], PARTS["range_small"])
    target = info.p[_points(info, rng, len(i))]
    d[i[large]] = (target[large] - o[i[large]]).astype(F)
    # every other small one is aimed too (normalised), or a sparse scene leaves them few hits
    aimed = ~large & ((i // 40) % 2 == 1)
    d[i[aimed]] = normalize((target[aimed] - o[i[aimed]]).astype(F)).astype(F)
    return _batch("range", o, d, part)


GENERATORS = {"interior": interior, "surface": surface, "scaled": scaled, "threshold": threshold,
              "range": range_}


def family(info: SceneInfo, name: str, scales=SCALES) -> Batch:
    if name == "mixed":
        return concat([family(info, f, scales) for f in FAMILIES], "mixed")
    if name == "scaled":
        return scaled(info, scales)
    return GENERATORS[name](info)


def concat(batches, name) -> Batch:
    nan = lambda b: np.full(len(b), np.nan, F) if b.tmax is None else b.tmax  # noqa: E731
    return Batch(name, np.concatenate([b.o for b in batches]),
                 np.concatenate([b.d for b in batches]),
                 np.concatenate([nan(b) for b in batches]),
                 np.concatenate([b.part for b in batches]),
                 np.concatenate([b.aux for b in batches]))


def permutation(b: Batch) -> np.ndarray:
    """The one seeded permutation every batch is also used under."""
    return np.random.default_rng(799).permutation(len(b))


def tmax_cycle(t):
    """tmax by ray index over {t, next above t, next below t, t/2, 2t, 0, -1, +inf, NaN}."""
    t = np.ascontiguousarray(t, F)
    with np.errstate(over="ignore", invalid="ignore"):
        choices = np.stack([t, np.nextafter(t, INF), np.nextafter(t, -INF), t / F(2), F(2) * t,
                            np.zeros_like(t), -np.ones_like(t), np.full_like(t, np.inf),
                            np.full_like(t, np.nan)])
    return choices[np.arange(len(t)) % 9, np.arange(len(t))]


def occlusion_tmax(b: Batch, t):
    """surface(c)'s own tmax (dist - eps); tmax_cycle of the oracle's t on every other ray."""
    cyc = tmax_cycle(t)
    if b.tmax is None:
        return cyc
    own = b.part == PARTS["surface_c"]
    return np.where(own, b.tmax, cyc).astype(F)


# ---------------------------------------------------------------- mix conditions
def det3(c1, c2, c3):
    return c1[:, 0] * (c2[:, 1] * c3[:, 2] - c3[:, 1] * c2[:, 2]) + \
        c2[:, 0] * (c3[:, 1] * c1[:, 2] - c1[:, 1] * c3[:, 2]) + \
        c3[:, 0] * (c1[:, 1] * c2[:, 2] - c2[:, 1] * c1[:, 2])


def quot_coord(x):
    a = np.abs(x)
    return (a == 0) | ((a >= F(2.0 ** -26)) & (a <= F(2.0 ** 48)))


def det_in_range(info: SceneInfo, b: Batch, rec, shape):
    """For the rays whose oracle hit is a triangle: is |det3(a1, a2, d)| inside tri_quotients'
    shared-reciprocal range [2^-40, 2^40]?  Returns (inside, outside) counts."""
    hit = (rec[:, 7] == 1.0) & (shape >= 0)
    tri = info.tri[np.where(hit, shape, 0)]
    hit &= ~np.isnan(tri[:, 0, 0])
    a1, a2 = tri[:, 0] - tri[:, 1], tri[:, 0] - tri[:, 2]
    with np.errstate(over="ignore", invalid="ignore"):
        det = np.abs(det3(a1, a2, b.d))
    inside = (det >= F(2.0 ** -40)) & (det <= F(2.0 ** 40))
    return int((hit & inside).sum()), int((hit & ~inside).sum())


def check_mix(info: SceneInfo, b: Batch, rec, shape):
    """Assert family `b.name`'s mix conditions from the oracle's records alone; returns the
    counts (for the log)."""
    hit, t = rec[:, 7] == 1.0, rec[:, 3]
    n = len(b)
    assert n <= 8192 or b.name == "mixed"
    got = {"rays": n, "hits": int(hit.sum())}
    if b.name == "interior":
        inside = ((b.o > info.lo) & (b.o < info.hi)).all(axis=1)
        waves = [len(np.unique(b.o[k:k + 64].view(np.uint32), axis=0)) for k in range(0, n, 64)]
        got.update(misses=int((~hit).sum()), inside=int(inside.sum()), distinct=min(waves))
        assert got["hits"] >= 1000 and got["misses"] >= 1000, got
        assert got["inside"] >= 1000 and got["distinct"] >= 32, got
    elif b.name == "surface":
        c = b.part == PARTS["surface_c"]
        with np.errstate(invalid="ignore"):
            occ = hit & (t > 0) & (t < b.tmax)
        bb = b.part == PARTS["surface_b"]
        on_start = hit & (shape == b.aux) & (t > 0)
        got.update(occluded=int((c & occ).sum()), unoccluded=int((c & ~occ).sum()),
                   self_hits=int((bb & on_start).sum()), self_misses=int((bb & ~on_start).sum()))
        assert got["occluded"] >= 300 and got["unoccluded"] >= 300, got
        assert got["self_hits"] >= 50 and got["self_misses"] >= 50, got
    elif b.name == "scaled":
        got["scales"] = len(np.unique(b.aux[:64]))
        assert all(len(np.unique(b.aux[k:k + 64])) == got["scales"] for k in range(0, n - 63, 64))
        assert got["scales"] >= 8
        if not np.isnan(info.tri[:, 0, 0]).all():  # (a scene of spheres has no det)
            got["det_inside"], got["det_outside"] = det_in_range(info, b, rec, shape)
            assert got["det_inside"] >= 100 and got["det_outside"] >= 100, got
    elif b.name == "threshold":
        small = np.abs(b.d) < EPS_SKIP
        i = np.arange(n)
        a = b.aux % 4
        oa, da = b.o[i, a], np.abs(b.d[i, a])
        outside = (oa < info.lo[a]) | (oa > info.hi[a])
        assert np.array_equal(outside, b.aux >= 4) and (a < 3).all()
        got.update(skipped_outside_hits=int((small[i, a] & outside & hit).sum()),
                   skipped_outside=int((small[i, a] & outside).sum()),
                   just_above=int(((da >= EPS_SKIP) & (da <= np.nextafter(EPS_SKIP, F(1)))).sum()),
                   inside=int((~outside).sum()), outside=int(outside.sum()))
        assert not small.all(axis=1).any()
        assert got["skipped_outside_hits"] >= 100 and got["just_above"] >= 100, got
        assert abs(got["inside"] - got["outside"]) <= 1
    elif b.name == "range":
        small = b.part == PARTS["range_small"]
        large = b.part == PARTS["range_large"]
        quot = quot_coord(b.o).all(axis=1)
        got["scene_quot_ok"] = info.quot_ok
        # LaneRay::quot = scene_quot_ok && ...: with a false scene flag no lane takes the
        # shared-reciprocal path and the family says nothing about it.  Only the 99-level tree
        # (v0 coordinates down to 2^-99; it is there for the spill stack) may be such a scene.
        assert info.quot_ok or info.name == "deep", got
        got.update(small_hits=int((small & hit).sum()), large=int(large.sum()),
                   large_hits=int((large & hit).sum()), quot_false=int((~quot).sum()))
        assert got["small_hits"] >= 200, got
        # each wave holds both values of LaneRay::quot
        assert all(0 < (~quot[k:k + 64]).sum() < 64 for k in range(0, n, 64)), got
        assert not quot[large].any() and quot[b.part == PARTS["range_plain"]].all()
    return got
