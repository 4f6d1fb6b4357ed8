"""Helpers of the light-sample tests (rt_shade_rays_lit*).

`restate`: the depth-0 shading of Scene::trace_ray (HW2/Scene.cpp:88-139) restated outside the
oracle, with the emitter term of HW3/src/Scene.cpp:207-218 added, because the oracle knows no
emitters.  One fp32 rounding per operation (numpy float32 arithmetic never contracts), the
oracle's operation order, `math.pow` for the fp64 pow; the loop runs over the lights, each
step over all rays at once.  The geometry is the oracle's: the hit from
OracleScene.intersect_rays, the material through rq_util.object_list, every shadow decision from
intersect_rays of the shadow ray with 0 < t < dist - eps.  test_lit_query_host.py earns it the
right to judge the emitter term: fed a scene's own point lights it equals OracleScene.shade_rays
bit for bit.  The emitter term itself is checked against a golden from HW3's compiled code: an
<AreaLight> whose every sample is its position (tests/test_ref_hw34_host.py).

Below it: light records, variant scenes with another light list, and the device launch."""
from __future__ import annotations

import math
import os

import numpy as np

import desc_xml
import rq_util

f32 = np.float32
NAN = f32(np.nan)


# ---------------------------------------------------------------- records
def records(position, intensity, normal=None):
    """LIGHT_SAMPLE_DTYPE records from (..., 3) positions and intensities (and normals)."""
    import ceng795_amd
    position = np.asarray(position, f32)
    out = np.zeros(position.shape[:-1], ceng795_amd.LIGHT_SAMPLE_DTYPE)
    out["position"] = position
    out["intensity"] = np.asarray(intensity, f32)
    if normal is not None:
        out["normal"] = np.asarray(normal, f32)
    return out


def scene_records(desc):
    """The scene's own point lights as shared records."""
    n = desc.d.num_lights
    return records([list(desc.lights[i].position) for i in range(n)],
                   [list(desc.lights[i].intensity) for i in range(n)])


def eighths(rng, lo, hi, shape):
    """Multiples of 1/8 in [lo, hi]: their decimal text parses back to exactly this fp32."""
    return (rng.integers(int(lo * 8), int(hi * 8) + 1, shape) / 8.0).astype(f32)


def write_with_lights(name, directory, tag, lights, change=None):
    """`name`'s scene (rigged as rq_util.scene_xml has it) with its light list replaced by
    `lights` [(position, intensity)], as <name>_<tag>.xml; asserts that the text reads back to
    the fp32 values given."""
    path = os.path.join(directory, f"{name}_{tag}.xml")
    if not os.path.exists(path):
        spec = spec_of(name)
        spec.lights = [(tuple(float(x) for x in p), tuple(float(x) for x in i)) for p, i in lights]
        if change:
            change(spec)
        tmp = path + ".tmp"
        with open(tmp, "w") as f:
            f.write(spec.to_xml())
        os.replace(tmp, path)
        back = desc_xml.Desc(path)
        assert back.d.num_lights == len(lights)
        for k, (p, i) in enumerate(lights):
            assert np.array_equal(np.array(list(back.lights[k].position), f32), np.asarray(p, f32))
            assert np.array_equal(np.array(list(back.lights[k].intensity), f32), np.asarray(i, f32))
    return path


def spec_of(name):
    import scenes
    if name == "deep":
        return rq_util.deep_scene()
    return {**scenes.CATALOGUE, **scenes.RECURSIVE}[name][0]()


def spec_lights(name):
    """The catalogue scene's own light list [(position, intensity)] as fp32 arrays (what the
    loader reads from the scene's text)."""
    return [(np.array(p, f32), np.array(i, f32)) for p, i in spec_of(name).lights]


# ---------------------------------------------------------------- the restatement
def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _length(a):
    return np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])


def _pow(c, e):
    return np.array([math.pow(float(x), float(y)) for x, y in zip(c, e)], np.float64).astype(f32)


def restate(xml, o, d, own, miss=None):
    """Depth-0 Scene::trace_ray of rays (o, d) with the light list `own`: LIGHT_SAMPLE_DTYPE
    records of shape (n, k), every ray with its own row, in order (nothing else is lit: pass the
    scene's point lights as records to have them).  `miss`: the colour of a miss (the background
    when depth 0 is the scene's maximum, else black).  Returns ((n, 4) {r, g, b, t or +inf},
    shadow rays cast)."""
    from oracle.cpu_ref import OracleScene
    desc = desc_xml.Desc(xml)
    objects = rq_util.object_list(desc)
    eps = f32(desc.d.shadow_ray_epsilon)
    ambient = np.array(list(desc.d.ambient_light), f32)
    if miss is None:
        miss = np.array(list(desc.d.background), f32) if desc.d.max_recursion_depth == 0 else \
            np.zeros(3, f32)
    o = np.ascontiguousarray(o, f32)
    d = np.ascontiguousarray(d, f32)
    n = len(o)
    orc = OracleScene(xml)
    rec, shape = orc.intersect_rays(o, d)
    hit = rec[:, 7] == 1.0
    idx = np.flatnonzero(hit)
    t = rec[idx, 3]
    nrm = rec[idx, 4:7]
    mat = np.array([objects[s][-1] for s in shape[idx]], np.int64)
    field = lambda name: np.array([list(getattr(desc.mats[m], name)) for m in  # noqa: E731
                                   range(desc.d.num_materials)], f32)[mat]
    ka, kd, ks = field("ambient"), field("diffuse"), field("specular")
    phong = np.array([desc.mats[m].phong_exponent for m in range(desc.d.num_materials)], f32)[mat]
    oh, dh = o[idx], d[idx]
    shadow_rays = 0
    with np.errstate(all="ignore"):
        p = oh + dh * t[:, None]                      # Ray::point_at
        w0v = oh - p
        w0 = w0v / _length(w0v)[:, None]
        color = np.zeros((len(idx), 3), f32) + ka * ambient[None, :]
        for j in range(own.shape[1]):
            L = own[idx, j]
            active = np.isfinite(L["position"]).all(axis=1)
            a = np.flatnonzero(active)
            if not len(a):
                continue
            pa = p[a]
            ld = L["position"][a] - pa
            dist = _length(ld)
            wi = ld / dist[:, None]
            so = pa + wi * eps
            srec, _ = orc.intersect_rays(so, wi)
            shadow_rays += len(a)
            st = srec[:, 3]
            occ = (srec[:, 7] == 1.0) & (st < (dist - eps)) & (st > f32(0))
            inten = L["intensity"][a]
            en = L["normal"][a]
            point = (en == 0).all(axis=1)
            ic = _dot(-wi, en)
            d2 = dist * dist
            cos_d = _dot(nrm[a], wi)
            kdi = kd[a] * inten
            kdi = np.where(point[:, None], kdi, kdi * ic[:, None])
            dif = (kdi * cos_d[:, None]) / d2[:, None]
            hv = w0[a] + wi
            cos_s = np.maximum(_dot(nrm[a], hv / _length(hv)[:, None]), f32(0))
            pw = _pow(cos_s, phong[a])
            ksi = ks[a] * inten
            ksi = np.where(point[:, None], ksi, ksi * ic[:, None])
            spe = (ksi * pw[:, None]) / d2[:, None]
            lit = a[~occ]
            color[lit] = (color[lit] + dif[~occ]) + spe[~occ]
    orc.close()
    out = np.zeros((n, 4), f32)
    out[:, :3] = miss[None, :]
    out[:, 3] = np.inf
    out[idx, :3] = f32(0) + color
    out[idx, 3] = t
    assert out.dtype == f32
    return out, shadow_rays


# ---------------------------------------------------------------- GPU launch
def shade_lit_device(s, o, d, lights, *, n=None, pad=0, stream=None, shared=False, **kw):
    """rt_shade_rays_lit_device over the first n rays (lights: (len(o), k) or shared (k,)); the
    output holds `pad` more slots of 0xA5 bytes.  Returns (radiance[n], the pad slots' bytes)."""
    import torch
    import ceng795_amd
    from ceng795_amd.scene import pack_lights
    rays = ceng795_amd.pack_rays(o, d)
    lit, k = pack_lights(lights, len(rays), shared)
    n = len(rays) if n is None else n
    dr = rq_util.to_device(rays) if len(rays) else torch.zeros(32, dtype=torch.uint8, device="cuda")
    dl = rq_util.to_device(lit) if lit.size else torch.zeros(48, dtype=torch.uint8, device="cuda")
    out = torch.full(((n + pad) * 16 + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream() if stream is None else stream
    torch.cuda.synchronize()  # the buffers were filled on the current stream
    with torch.cuda.stream(st):
        s.shade_rays_lit_device(dr.data_ptr(), n, dl.data_ptr(), k, out.data_ptr(), shared=shared,
                                stream=st.cuda_stream, **kw)
    st.synchronize()
    raw = out.cpu().numpy()
    return raw[:n * 16].view(ceng795_amd.RADIANCE_DTYPE).copy(), raw[n * 16:(n + pad) * 16]
