"""Goldens from the reference's own compiled HW3 / HW4 code.

The helpers of the later features (smooth_util, instance_util, motion_util, lit_util, texture_util)
are numpy restatements by the hand that wrote the kernels.  Here is what puts both before the
reference itself: the scenes those helpers' writers produce, a ray batch per scene, and the
records of oracle/_ref/hw3_harness and hw4_harness (oracle/ref/hw34_harness.cpp: the unmodified
HW3 / HW4 sources) for them, stored by tests/golden/make_golden_hw3.py and make_golden_hw4.py.

  cases            HW3_CASES / HW4_CASES -> build(name, directory): a Case (scene file, rays).
  harness          hits / trace / texels / normals of a Case; every command runs twice and must
                   give the same bytes (the reference seeds mt19937 from the clock where it samples).
  restatement      restate(case): what the helpers say for the same rays, in the goldens' fields.
  departures       CLASSES: where the library is knowingly not the homework the golden comes from.
                   tree_classes(case) decides a ray's membership from the objects its restated
                   ray tree meets (materials, kinds, lookups) — never from a colour.
"""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import tempfile
from dataclasses import dataclass, field

import numpy as np

import instance_util as iu
import motion_util as mu
import rq_util
import smooth_util as su
import texture_util as tu

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
HARNESS = {3: os.path.join(ROOT, "oracle", "_ref", "hw3_harness"),
           4: os.path.join(ROOT, "oracle", "_ref", "hw4_harness")}

HIT_DTYPE = np.dtype([("hit", np.int32), ("t", F), ("normal", F, 3), ("material", np.int32),
                      ("u", F), ("v", F), ("texture", np.int32), ("zero", np.int32)])

# Where the library departs from the homework a golden comes from: (bit, name, the reference line).
# A ray is in a class when its restated tree holds what the class names.
BEER, SPHERE4, PAST_IMAGE, PLAIN_MESH = 1, 2, 4, 8
CLASSES = {
    BEER: ("Beer's law: HW2's sign",
           "HW3/src/Scene.cpp:292-294 and HW4/src/Scene.cpp:323-325 have exp(log(T) * t); the "
           "library keeps HW2/Scene.cpp:166-168's exp(-log(T) * t).  In the class: a tree that "
           "meets a material whose Transparency has a component other than 0 and 1."),
    SPHERE4: ("spheres: HW3's, not HW4's transformed sphere",
              "HW4/src/Sphere.cpp:31-98 sends every sphere through its (identity) transformation "
              "and normalises the unit normal once more (:95); the library's sphere is HW3's.  In "
              "the class: a tree of an HW4 golden that meets a sphere at a point where N / |N| "
              "differs from N."),
    PAST_IMAGE: ("clamped bilinear: reads past the image are skipped",
                 "HW4/src/Texture.cpp:120-123 reads texel (qn, pn = w) for qn = h - 1: index 3 w h, "
                 "past the image.  The library skips that term.  In the class: a tree with a "
                 "clamped bilinear lookup whose guarded index reaches 3 w h."),
    PLAIN_MESH: ("meshes outside instanced scenes: HW2's Mesh, not HW3's identity Mesh_instance",
                 "HW3 and HW4 wrap every <Mesh> in a Mesh_instance whose intersect normalises the "
                 "unit normal once more (include/Mesh.h:63-66, HW4 :74-76); outside instanced scenes "
                 "the library's mesh is HW2's and keeps Hit_data::normal as the triangle gave it.  In "
                 "the class: a tree that meets a mesh face at a point where N / |N| differs from N."),
}
MAX_EXCLUDED = 0.2  # at most one fifth of a scene's rays outside the colour comparison


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def sha256_file(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


# ---------------------------------------------------------------- the cases
@dataclass
class Case:
    name: str
    hw: int
    kind: str                 # "smooth" | "textured" | "instanced" | "moving"
    xml: str                  # the file the reference and the library's loader read
    o: np.ndarray
    d: np.ndarray
    time: np.ndarray
    plain_xml: str = None     # smooth / textured: the file the CPU oracle reads (no HW4 tags)
    scene: dict = field(default_factory=dict)   # smooth / textured: TexTracer's arguments
    images: dict = None       # textured: name -> (h, w, 3) uint8
    spec: object = None       # instanced / moving: the InstSpec / MotionSpec of the file
    area: dict = None         # the tiny area light: position, intensity, normal


def shell_rays(n, seed, centre, extent, radius):
    """Rays from a shell of `radius` around `centre` toward seeded points of the box centre +-
    extent; directions are not normalised."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    o = (np.asarray(centre) + radius * v / np.linalg.norm(v, axis=1)[:, None]).astype(F)
    target = (np.asarray(centre) + rng.uniform(-1, 1, size=(n, 3)) * np.asarray(extent)).astype(F)
    return o, (target - o).astype(F)


def _camera_and_shell(xml, seed, centre, extent, radius, shell=320):
    b = rq_util.oracle_batch(xml, cameras=[0])
    o, d = shell_rays(shell, seed, centre, extent, radius)
    return np.concatenate([b.o, o]), np.concatenate([b.d, d])


def _zero_time(o):
    return np.zeros(len(o), F)


# 2^-27: position + e1 eps1 + e2 eps2 (HW3/src/Scene.cpp:197-199, eps in [0, 1)) rounds back to
# `position` in each of its two additions: every component of the position has magnitude >= 1, so
# its fp32 spacing is >= 2^-23, and |e eps| < 2^-27 is below half of that (2^-24); a zero component
# of an edge adds exactly 0.  The cross product of the edges is (0, -2^-54, 0), its length 2^-54
# exactly, so the emitter normal is (0, -1, 0) exactly.  The two-run check of the generator would
# show a sample that moved.
AREA_EDGE = "7.450580596923828e-09"
AREA = dict(position=(-3.0, 6.0, 2.0), intensity=(3000.0, 2500.0, 2000.0), normal=(0.0, -1.0, 0.0))


def _area_edit(text):
    p, i = AREA["position"], AREA["intensity"]
    light = (f'    <AreaLight id="1">\n      <Position>{p[0]} {p[1]} {p[2]}</Position>\n'
             f'      <Intensity>{i[0]} {i[1]} {i[2]}</Intensity>\n'
             f'      <EdgeVector1>{AREA_EDGE} 0 0</EdgeVector1>\n'
             f'      <EdgeVector2>0 0 {AREA_EDGE}</EdgeVector2>\n    </AreaLight>\n')
    assert text.count("  </Lights>") == 1
    return text.replace("  </Lights>", light + "  </Lights>")


def _smooth_case(name, directory, base, clear=False, area=False):
    factory, smooth = su.CASES[base]
    spec = factory()
    if clear:
        for m in spec.materials:
            if m.transparency is not None:
                m.transparency = (1, 1, 1)
    plain = su.write_spec(spec, directory, name + "_plain" if area else name, smooth)
    xml = plain
    if area:  # the CPU oracle's loader knows no <AreaLight>: it reads the plain file
        xml = os.path.join(directory, name + ".xml")
        with open(xml, "w") as f:
            f.write(_area_edit(open(plain).read()))
    centre, extent, radius = {"sm_mixed": ((-5.0, 1.5, 0.2), (4.0, 3.5, 0.6), 9.0),
                              "sm_glass": ((0.0, 0.0, 0.0), (2.2, 1.2, 1.2), 6.0)}[base]
    o, d = _camera_and_shell(plain, 31, centre, extent, radius)
    return Case(name, 3, "smooth", xml, o, d, _zero_time(o), plain_xml=plain,
                scene=dict(smooth=smooth), area=AREA if area else None)


def _strip_triangle_texture(text):
    at = text.index('<Triangle id="1"')
    s = text.index("\n      <Texture>", at)
    e = text.index("</Texture>", s) + len("</Texture>")
    assert e < text.index("</Triangle>", at)
    return text[:s] + text[e:]


OLD_GLASS = "<Transparency>0.9 0.8 0.7</Transparency>"
CLEAR_GLASS = "<Transparency>1 1 1</Transparency>"


def write_ppm(path, rgb8):
    """A binary PPM: stb_image goes by the content, whatever the file is called."""
    h, w = rgb8.shape[:2]
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(np.ascontiguousarray(rgb8, np.uint8).tobytes())


def _textured_case(name, directory, clear=False):
    """tx_mixed as HW4 reads it, without the loose triangle's <Texture> (HW4's loose triangle
    leaves Hit_data::u, v unwritten: the library's triangle_texture is its own extension)."""
    def change(text):
        text = _strip_triangle_texture(text)
        if clear:
            assert text.count(OLD_GLASS) == 1
            text = text.replace(OLD_GLASS, CLEAR_GLASS)
        return text
    xml, images, scene = tu.textured_xml(directory, name, change=change)
    scene = dict(scene, triangle_texture=[-1])
    plain = tu.mixed_scene(directory)[0]
    if clear:
        text = open(plain).read()
        assert text.count(OLD_GLASS) == 1
        plain = os.path.join(directory, name + "_plain.xml")
        with open(plain, "w") as f:
            f.write(text.replace(OLD_GLASS, CLEAR_GLASS))
    for k, img in images.items():
        write_ppm(os.path.join(directory, k), img)
    o, d = _camera_and_shell(plain, 41, (0.0, 0.5, -0.5), (3.0, 1.7, 2.0), 7.0)
    return Case(name, 4, "textured", xml, o, d, _zero_time(o), plain_xml=plain, scene=scene,
                images=images)


def _block(text, tag):
    a = text.index(f"  <{tag}>")
    return a, text.index(f"</{tag}>", a) + len(tag) + 3


def moving_edit(text):
    from test_motion_host import _moving_edit
    return _moving_edit(text)


def _instanced_case(name, directory, shiny=False, moving=False):
    """instance_util.xml_three, optionally with scene_shiny's materials, lights and depth (the glass
    clear: Transparency 1 1 1) or with test_motion_host's <MotionBlur> tags."""
    import ceng795_amd
    donor = iu.scene_shiny()
    donor.materials[4].transparency = (1, 1, 1)
    donor_text = donor._spec(donor.meshes, donor.triangles, donor.spheres).to_xml()

    def shine(text):
        for tag in ("Lights", "Materials"):
            a, b = _block(text, tag)
            c, e = _block(donor_text, tag)
            text = text[:a] + donor_text[c:e] + text[b:]
        assert text.count("<MaxRecursionDepth>0</MaxRecursionDepth>") == 1
        text = text.replace("<MaxRecursionDepth>0</MaxRecursionDepth>",
                            "<MaxRecursionDepth>3</MaxRecursionDepth>")
        for old, new in (('resetTransform="true">\n      <Material>3</Material>', "4"),
                         ('baseMeshId="1">\n      <Material>2</Material>', "5")):
            assert text.count(old) == 1
            text = text.replace(old, old[:old.index("<Material>")] + f"<Material>{new}</Material>")
        return text

    plain, _ = iu.xml_three(directory, shine if shiny else None, tag=name + ("_still" if moving else ""))
    mesh, mat, xf = ceng795_amd.host_instances_xml(plain)
    base = donor if shiny else iu.scene_three()
    instances = [(int(m), int(k), x) for m, k, x in zip(mesh, mat, xf)]
    if moving:
        xml, _ = iu.xml_three(directory, moving_edit, tag=name)
        vel, sxf, svel = ceng795_amd.host_motion_xml(xml)
        spec = mu.MotionSpec(base.vertices, base.meshes, instances, triangles=base.triangles,
                             spheres=base.spheres, materials=base.materials,
                             velocity=[tuple(v) for v in vel], sphere_xf=list(sxf),
                             sphere_vel=[tuple(v) for v in svel])
        o, d, time = mu.main_batch()
        co, cd = iu.camera_rays(17, 9)
        o, d = np.concatenate([o, co]), np.concatenate([d, cd])
        time = np.concatenate([time, np.resize(mu.SPECIAL_TIMES, len(co))]).astype(F)
    else:
        xml = plain
        spec = iu.InstSpec(base.vertices, base.meshes, instances, triangles=base.triangles,
                           spheres=base.spheres, materials=base.materials, lights=base.lights,
                           max_depth=base.max_depth)
        co, cd = iu.camera_rays(33, 31) if shiny else iu.camera_rays(17, 9)
        ro, rd = iu.random_rays(400, 77)
        o, d = np.concatenate([co, ro]), np.concatenate([cd, rd])
        time = _zero_time(o)
    spec.write(directory, name + "_desc")
    return Case(name, 3, "moving" if moving else "instanced", xml, o, d, time, spec=spec)


HW3_CASES = {
    "sm_mixed": lambda d: _smooth_case("sm_mixed", d, "sm_mixed"),
    "sm_area": lambda d: _smooth_case("sm_area", d, "sm_mixed", area=True),
    "sm_glass": lambda d: _smooth_case("sm_glass", d, "sm_glass"),
    "sm_clear": lambda d: _smooth_case("sm_clear", d, "sm_glass", clear=True),
    "xml_three": lambda d: _instanced_case("ref_three", d),
    "xml_shiny": lambda d: _instanced_case("ref_shiny", d, shiny=True),
    "xml_moving": lambda d: _instanced_case("ref_moving", d, moving=True),
}
HW4_CASES = {
    "tx_mixed": lambda d: _textured_case("tx_ref_mixed", d),
    "tx_clear": lambda d: _textured_case("tx_ref_clear", d, clear=True),
}
CASES = {3: HW3_CASES, 4: HW4_CASES}
_BUILT = {}


def build(hw, name, directory) -> Case:
    key = (hw, name, directory)
    if key not in _BUILT:
        c = CASES[hw][name](directory)
        for a in (c.o, c.d, c.time):
            a.setflags(write=False)
        _BUILT[key] = c
    return _BUILT[key]


# ---------------------------------------------------------------- the harness
def _run(hw, cmd, xml, payload, extra=()):
    """One harness command, twice: the bytes it wrote, which must not differ between the runs."""
    outs = []
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "in.bin")
        if payload is not None:
            with open(src, "wb") as f:
                f.write(payload)
        for k in range(2):
            dst = os.path.join(tmp, f"out{k}.bin")
            args = [HARNESS[hw], cmd, xml] + ([src] if payload is not None else []) + [dst, *extra]
            subprocess.run(args, check=True, stdout=subprocess.DEVNULL, cwd=os.path.dirname(xml))
            with open(dst, "rb") as f:
                outs.append(f.read())
    assert outs[0] == outs[1], f"hw{hw}_harness {cmd} {os.path.basename(xml)}: two runs differ"
    return outs[0]


def _rays(o, d, time):
    return np.concatenate([o, d, np.asarray(time, F)[:, None]], axis=1).astype(F)


def ref_hits(case_or_hw, xml=None, o=None, d=None, time=None):
    c = case_or_hw
    hw, xml, o, d, time = (c.hw, c.xml, c.o, c.d, c.time) if isinstance(c, Case) else (c, xml, o, d, time)
    return np.frombuffer(_run(hw, "hits", xml, _rays(o, d, time).tobytes()), HIT_DTYPE).copy()


def ref_trace(case, in_medium=False, depth=None):
    rec = np.zeros((len(case.o), 8), F)
    rec[:, :7] = _rays(case.o, case.d, case.time)
    rec.view(np.int32)[:, 7] = int(in_medium)
    extra = () if depth is None else (str(depth),)
    return np.frombuffer(_run(case.hw, "trace", case.xml, rec.tobytes(), extra), F).reshape(-1, 3).copy()


def ref_texels(xml, k, u, v):
    q = np.zeros((len(u), 3), F)
    q.view(np.int32)[:, 0] = k
    q[:, 1], q[:, 2] = u, v
    return np.frombuffer(_run(4, "texels", xml, q.tobytes()), F).reshape(-1, 3).copy()


def ref_normals(case):
    raw = np.frombuffer(_run(case.hw, "normals", case.xml, None), np.uint8).reshape(-1, 16)
    return raw[:, :4].copy().view(np.int32).reshape(-1) != 0, raw[:, 4:].copy().view(F).reshape(-1, 3)


# ---------------------------------------------------------------- texel queries
def past_image(tex, u, v):
    """Does Texture::get_color_at(u, v) read at index 3 w h or beyond?  From the reference's own
    index arithmetic (HW4/src/Texture.cpp:58-68, 102-111) and the guards of the reads (:115-129),
    in fp32 as it runs; only the clamped bilinear form can."""
    if tex["interpolation"] != tu.BILINEAR or tex["appearance"] != tu.CLAMP:
        return False
    h, w = int(tex["rgb8"].shape[0]), int(tex["rgb8"].shape[1])
    with np.errstate(all="ignore"):
        x = tu._fmax(F(0), tu._fmin(F(1), F(u)))
        y = tu._fmax(F(0), tu._fmin(F(1), F(v)))
        x = F(x * F(w))
        if x >= F(w):
            x = F(x - F(1))
        y = F(y * F(h))
        if y >= F(h):
            y = F(y - F(1))
        p, q = int(x), int(y)
        pn, qn = p + 1, int(F(y + F(1)))
    reads = [3 * (w * q + p) + 2]
    if pn < w:
        reads.append(3 * (w * q + pn) + 2)
    if qn < h:
        reads.append(3 * (w * qn + pn) + 2)
    if pn < w and qn < h:
        reads.append(3 * (w * qn + p) + 2)
    return max(reads) >= 3 * w * h


def texel_textures():
    """The textures of the lookup grids: every size of texture_util.SIZES in every mode of MODES,
    images seeded as test_gpu_textures.test_device_lookup seeds them."""
    out = []
    for w, h in tu.SIZES:
        for k, (i, a) in enumerate(tu.MODES):
            out.append(tu.random_texture(w, h, 100 * w + 10 * h + k, interpolation=i, appearance=a))
    return out


def texel_scene(directory):
    """tx_mixed's file with its <Textures> block replaced by texel_textures(), images as PPM."""
    textures = texel_textures()
    block = ["  <Textures>"]
    for k, tex in enumerate(textures):
        write_ppm(os.path.join(directory, f"grid{k}.png"), tex["rgb8"])
        block += [f'    <Texture id="{k + 1}">', f"      <ImageName>grid{k}.png</ImageName>",
                  f"      <Interpolation>{tu._INTERPOLATION[tex['interpolation']]}</Interpolation>",
                  f"      <DecalMode>{tu._DECAL[tex['decal']]}</DecalMode>",
                  f"      <Appearance>{tu._APPEARANCE[tex['appearance']]}</Appearance>",
                  "    </Texture>"]
    block.append("  </Textures>")

    def change(text):
        a, b = _block(text, "Textures")
        return text[:a] + "\n".join(block) + text[b:]
    xml, images, _ = tu.textured_xml(directory, "tx_ref_grids", change=change)
    for k, img in images.items():
        write_ppm(os.path.join(directory, k), img)
    return xml, textures


def texel_queries(textures):
    """(k, u, v) of every grid query, and which of them read past the image."""
    ks, us, vs = [], [], []
    for k, tex in enumerate(textures):
        h, w = tex["rgb8"].shape[:2]
        u, v = tu.grid_queries(w, h)
        ks.append(np.full(len(u), k, np.int32))
        us.append(u)
        vs.append(v)
    k, u, v = np.concatenate(ks), np.concatenate(us).astype(F), np.concatenate(vs).astype(F)
    past = np.array([past_image(textures[a], b, c) for a, b, c in zip(k, u, v)], bool)
    return k, u, v, past


# ---------------------------------------------------------------- the restatement
class _Recorder:
    """Notes the `shape` ids of every hit a tracer shades (its hit_normals sees each level's)."""

    def __init__(self, tr):
        self.shapes, self.moved = [], []
        inner = tr.hit_normals

        def hook(o, d, rec, shape, idx):
            nrm = inner(o, d, rec, shape, idx)
            self.shapes.append(np.asarray(shape)[idx].copy())
            self.moved.append(renormalising_moves(nrm))
            return nrm
        tr.hit_normals = hook

    def take(self):
        """(the shapes shaded since the last call, whether N / |N| differs from N at each)."""
        out = np.concatenate(self.shapes) if self.shapes else np.zeros(0, np.int64)
        moved = np.concatenate(self.moved) if self.moved else np.zeros(0, bool)
        self.shapes, self.moved = [], []
        return out, moved


def renormalising_moves(nrm):
    """Per normal: does Vector3::normalize of it change a bit?"""
    with np.errstate(all="ignore"):
        again = su._normalize(np.ascontiguousarray(nrm, F))
    return (bits(again) != bits(nrm)).any(axis=1)


def _departing(kt):
    """Materials whose Transparency has a component other than 0 and 1."""
    return ((kt != 0) & (kt != 1)).any(axis=1)


def tex_tracer(case):
    sc = case.scene
    return tu.TexTracer(case.plain_xml, textures=sc.get("textures", ()), mesh_texture=sc.get("mesh_texture"),
                        triangle_texture=sc.get("triangle_texture"), sphere_texture=sc.get("sphere_texture"),
                        uv=sc.get("uv"), smooth=sc.get("smooth", ()))


def composite(case):
    return mu.MotionComposite(case.spec) if case.kind == "moving" else iu.Composite(case.spec)


def possible_classes(case, kt, has_sphere):
    """The classes some ray of the case could be in."""
    out = BEER if _departing(kt).any() else 0
    if case.kind in ("smooth", "textured"):
        out |= PLAIN_MESH
    if case.hw == 4:
        if has_sphere:
            out |= SPHERE4
        if any(t["interpolation"] == tu.BILINEAR and t["appearance"] == tu.CLAMP
               for t in case.scene.get("textures", ())):
            out |= PAST_IMAGE
    return out


def tree_classes(case, rays=None):
    """uint8 per ray: the departure classes its restated tree is in (rays: indices, None: all).
    Each ray is traced alone, so what the tracer shaded in between is that ray's tree."""
    idx = np.arange(len(case.o)) if rays is None else np.asarray(rays)
    out = np.zeros(len(idx), np.uint8)
    none = np.zeros(1, bool)
    with np.errstate(all="ignore"):
        if case.kind in ("smooth", "textured"):
            tr = tex_tracer(case)
            if possible_classes(case, tr.kt, (~tr.ob.tri).any()):
                rec = _Recorder(tr)
                bad = _departing(tr.kt)
                for j, i in enumerate(idx):
                    tr.lookups = []
                    tr.trace(case.o[i:i + 1], case.d[i:i + 1], none, tr.max_depth)
                    shapes, moved = rec.take()
                    cls = BEER if bad[tr.ob.mat[shapes]].any() else 0
                    if (moved & (tr.ob.mesh[shapes] >= 0)).any():
                        cls |= PLAIN_MESH
                    if case.hw == 4:
                        if (moved & ~tr.ob.tri[shapes]).any():
                            cls |= SPHERE4
                        if any(past_image(tr.textures[k], u, v) for k, u, v in tr.lookups):
                            cls |= PAST_IMAGE
                    out[j] = cls
            tr.close()
        else:
            comp = composite(case)
            tr = iu._tracer_class()(comp)
            if possible_classes(case, tr.kt, False):
                rec = _Recorder(tr)
                bad = _departing(tr.kt)
                for j, i in enumerate(idx):
                    if case.kind == "moving":
                        comp.set_time(F(case.time[i]))
                    tr.trace(case.o[i:i + 1], case.d[i:i + 1], none, tr.max_depth)
                    out[j] = BEER if bad[rec.take()[0]].any() else 0  # (shape = the material here)
            comp.close()
    return out


def homework(hw):
    """Context manager: the restatements as the homework has it where the library departs —
    Beer's factor with HW3's and HW4's sign, exp(log(T) t); the normal of every mesh face (HW4:
    and of every sphere) normalised once more.  With it the restatements must equal the goldens
    on the rays of those classes too, which shows that the classes are the whole difference."""
    import contextlib
    import math

    def beer(T, t):
        def one(x, y):
            try:
                lg = math.log(x) if x != 0.0 else -math.inf
            except ValueError:
                lg = math.nan
            try:
                return math.exp(lg * y)
            except OverflowError:
                return math.inf
        return np.array([one(float(x), float(y)) for x, y in zip(T, t)], np.float64).astype(F)

    plain_normals = su.Tracer.hit_normals

    def hit_normals(self, o, d, rec, shape, idx):
        nrm = plain_normals(self, o, d, rec, shape, idx)
        s = np.asarray(shape)[idx]
        again = self.ob.mesh[s] >= 0
        if hw == 4:
            again |= ~self.ob.tri[s]
        with np.errstate(all="ignore"):
            nrm[again] = su._normalize(nrm[again])
        return nrm

    @contextlib.contextmanager
    def patched():
        old = su._beer, tu._beer
        su._beer = tu._beer = beer
        su.Tracer.hit_normals = hit_normals
        try:
            yield
        finally:
            su._beer, tu._beer = old
            su.Tracer.hit_normals = plain_normals
    return patched()


def restate(case):
    """The helpers' answers for the case's rays in the goldens' fields: hit, t, normal, material,
    u, v, texture, rgb, rgb_medium (colours as Scene::trace_ray returns them at the scene's depth),
    near (texture_util's flag: a sphere lookup of the tree near an fp32 rounding boundary)."""
    o, d = np.ascontiguousarray(case.o), np.ascontiguousarray(case.d)
    n = len(o)
    out = dict(u=np.zeros(n, F), v=np.zeros(n, F), texture=np.full(n, -1, np.int32),
               near=np.zeros(n, bool))
    with np.errstate(all="ignore"):
        if case.kind in ("smooth", "textured"):
            tr = tex_tracer(case)
            rec, shape = tr.orc.intersect_rays(o, d)
            hit = rec[:, 7] == 1.0
            idx = np.flatnonzero(hit)
            out["hit"], out["t"] = hit, np.where(hit, rec[:, 3], F(0)).astype(F)
            out["normal"] = np.zeros((n, 3), F)
            out["normal"][idx] = tr.hit_normals(o, d, rec, shape, idx)
            out["material"] = np.where(hit, tr.ob.mat[np.where(hit, shape, 0)], -1).astype(np.int32)
            if case.kind == "textured":
                tid = tr.obj_tex[shape[idx]]
                tr.lookups = []
                p = o[idx] + d[idx] * rec[idx, 3][:, None]
                tr.texture_step(o, d, rec, shape, idx, p, "primary")
                tx = idx[tid >= 0]
                assert len(tr.lookups) == len(tx)
                out["texture"][tx] = tid[tid >= 0]
                out["u"][tx] = [a[1] for a in tr.lookups]
                out["v"][tx] = [a[2] for a in tr.lookups]
            for key, medium in (("rgb", False), ("rgb_medium", True)):
                out[key], _, _, near, _ = tu.trace(case.plain_xml, o, d, -1, medium, tracer=tr)
                out["near"] = out.get("near", False) | near
            if case.area:
                out["rgb"] = restate_area(case)
            tr.close()
        else:
            comp = composite(case)
            ref = comp.intersect(o, d, case.time) if case.kind == "moving" else comp.intersect(o, d)
            out["hit"], out["t"] = ref.hit, np.where(ref.hit, ref.t, F(0)).astype(F)
            out["normal"] = np.where(ref.hit[:, None], ref.normal, F(0)).astype(F)
            out["material"] = np.where(ref.hit, ref.material, -1).astype(np.int32)
            for key, medium in (("rgb", False), ("rgb_medium", True)):
                if case.kind == "moving":
                    out[key] = mu.trace_at(comp, o, d, case.time, -1, medium)[0]
                else:
                    out[key] = iu.trace(comp, o, d, -1, medium)[0]
            comp.close()
    return out


def area_records(case, desc=None):
    """(n, k) light records: the scene's point lights, then the tiny area light's one sample."""
    import desc_xml
    import lit_util
    desc = desc or desc_xml.Desc(case.plain_xml)
    own = lit_util.scene_records(desc)
    a = case.area
    one = lit_util.records([a["position"]], [a["intensity"]], [a["normal"]])
    row = np.concatenate([own, one])
    return np.broadcast_to(row, (len(case.o), len(row))).copy()


def area_record(case):
    """The area light's sample alone, for a shared record after the scene's own lights."""
    import lit_util
    a = case.area
    return lit_util.records([a["position"]], [a["intensity"]], [a["normal"]])


def restate_area(case):
    """Scene::trace_ray at depth 0 with the area light (HW3/src/Scene.cpp:184-230 after the point
    lights): smooth_util.restate_lit fed the scene's lights and the emitter record."""
    out = su.restate_lit(case.plain_xml, case.o, case.d, area_records(case),
                         smooth=case.scene.get("smooth", ()))[0]
    return np.ascontiguousarray(out[:, :3])


# ---------------------------------------------------------------- golden files
FIELDS = ("o", "d", "time", "hit", "t", "normal", "material", "u", "v", "texture", "rgb",
          "rgb_medium", "cls", "near")


def reference_records(case):
    """The harness records of a case in the goldens' fields (no `cls`)."""
    h = ref_hits(case)
    hit = h["hit"] == 1
    out = dict(o=case.o, d=case.d, time=case.time, hit=hit.astype(np.uint8), t=h["t"],
               normal=h["normal"], material=h["material"].astype(np.int16), u=h["u"], v=h["v"],
               texture=h["texture"].astype(np.int8), rgb=ref_trace(case, False),
               rgb_medium=ref_trace(case, True))
    assert (h["zero"] == 0).all()
    return out


def load(hw):
    """(arrays, summary) of golden_hw<hw>.npz / .json."""
    z = np.load(os.path.join(GOLDEN, f"golden_hw{hw}.npz"))
    with open(os.path.join(GOLDEN, f"golden_hw{hw}.json")) as f:
        return z, json.load(f)


def golden_case(z, name):
    return {k: z[f"{name}__{k}"] for k in FIELDS}


def normal_rows_excluded(normal, cls):
    """Hits outside the normal comparison: rays of a renormalisation class whose own first-hit
    normal N / |N| would move (`normal`: the un-renormalised one under test).  Wider than needed
    only for a first hit on a loose triangle or an HW3 sphere (never renormalised) whose tree is in
    such a class further down."""
    return ((cls & (PLAIN_MESH | SPHERE4)) != 0) & renormalising_moves(normal)


def colour_rows(g):
    """Rays inside the colour comparison: outside every departure class."""
    return g["cls"] == 0


def class_counts(cls):
    return {CLASSES[b][0]: int(((cls & b) != 0).sum()) for b in CLASSES}


# ---------------------------------------------------------------- the generator
def generate(hw, directory):
    """Everything make_golden_hw<hw>.py stores: (arrays, summary).  Runs the harness (each command
    twice), derives the departure classes from the restated trees and holds the two to each other:
    outside the classes the restatement equals the reference bit for bit, hits on every ray."""
    arrays, summary = {}, {"harness": f"hw{hw}_harness", "classes": {str(b): list(v) for b, v in CLASSES.items()},
                           "scenes": {}}
    for name in CASES[hw]:
        case = build(hw, name, directory)
        rec = reference_records(case)
        rec["cls"] = tree_classes(case)
        excluded = int((rec["cls"] != 0).sum())
        assert excluded <= MAX_EXCLUDED * len(case.o), (name, excluded)
        rec["near"] = np.zeros(len(case.o), np.uint8)
        rec["near"] = check_restatement(case, rec)["near"].astype(np.uint8)
        for k in FIELDS:
            arrays[f"{name}__{k}"] = np.ascontiguousarray(rec[k])
        files = {"xml": sha256_file(case.xml)}
        if case.plain_xml and case.plain_xml != case.xml:
            files["plain_xml"] = sha256_file(case.plain_xml)
        summary["scenes"][name] = {
            "sha256": files, "kind": case.kind, "rays": len(case.o), "hits": int(rec["hit"].sum()),
            "rays_compared_in_hits": len(case.o), "rays_compared_in_colour": len(case.o) - excluded,
            "excluded": class_counts(rec["cls"])}
        if case.kind in ("smooth", "textured"):
            has, vn = ref_normals(case)
            arrays[f"{name}__vn_has"] = has.astype(np.uint8)
            arrays[f"{name}__vn"] = vn
        print(name, json.dumps(summary["scenes"][name]), flush=True)
    if hw == 4:
        xml, textures = texel_scene(directory)
        k, u, v, past = texel_queries(textures)
        keep = ~past
        arrays["texels__k"], arrays["texels__u"], arrays["texels__v"] = k[keep], u[keep], v[keep]
        arrays["texels__rgb"] = ref_texels(xml, k[keep], u[keep], v[keep])
        summary["texels"] = {"sha256": {"xml": sha256_file(xml)}, "queries": int(keep.sum()),
                             "dropped_past_the_image": int(past.sum())}
        # the uv of every textured golden hit, through the reference's lookup of that texture
        for name in CASES[hw]:
            case = build(hw, name, directory)
            tex = arrays[f"{name}__texture"]
            sel = np.flatnonzero(tex >= 0)
            gu, gv = arrays[f"{name}__u"][sel], arrays[f"{name}__v"][sel]
            gone = np.array([past_image(case.scene["textures"][t], a, b)
                             for t, a, b in zip(tex[sel], gu, gv)], bool)
            sel = sel[~gone]
            arrays[f"{name}__texel_ray"] = sel.astype(np.int32)
            arrays[f"{name}__texel"] = ref_texels(case.xml, tex[sel].astype(np.int32),
                                                  arrays[f"{name}__u"][sel], arrays[f"{name}__v"][sel])
            summary["scenes"][name]["hit_texels"] = int(len(sel))
            summary["scenes"][name]["hit_texels_dropped_past_the_image"] = int(gone.sum())
        print("texels", json.dumps(summary["texels"]), flush=True)
    return arrays, summary


def check_restatement(case, g, homework_too=True):
    """The helpers against a case's golden records `g` (with `cls`), bit for bit: hits on every
    ray (the normal outside the two renormalisation classes, where the hit itself is in them),
    colours outside every class; then, restated as the homework has it, everything on every ray
    but the colours of PAST_IMAGE trees (the reference reads its heap there).  Returns the
    restatement's records."""
    mine = restate(case)
    hit = g["hit"].astype(bool)
    assert np.array_equal(mine["hit"], hit), case.name
    for k in ("t", "u", "v"):
        assert np.array_equal(bits(mine[k]), bits(g[k])), (case.name, k)
    assert np.array_equal(mine["material"], g["material"]) and np.array_equal(mine["texture"], g["texture"]), case.name
    same = (bits(mine["normal"]) == bits(g["normal"])).all(axis=1)
    assert same[~normal_rows_excluded(mine["normal"], g["cls"])].all(), (case.name, "normal")
    keep = g["cls"] == 0
    for k in ("rgb", "rgb_medium"):
        assert np.array_equal(bits(mine[k][keep]), bits(g[k][keep])), (case.name, k)
    if not homework_too or case.kind in ("instanced", "moving"):  # (nothing of it reaches those)
        return mine
    with homework(case.hw):
        theirs = restate(case)
    assert np.array_equal(bits(theirs["normal"]), bits(g["normal"])), (case.name, "homework normal")
    keep = (g["cls"] & PAST_IMAGE) == 0
    for k in ("rgb", "rgb_medium"):
        assert np.array_equal(bits(theirs[k][keep]), bits(g[k][keep])), (case.name, "homework", k)
    return mine


def write_golden(hw):
    if not os.path.exists(HARNESS[hw]):
        raise SystemExit(f"reference harness missing: run `make -C oracle ref-hw{hw}` first")
    with tempfile.TemporaryDirectory() as d:
        arrays, summary = generate(hw, d)
    path = os.path.join(GOLDEN, f"golden_hw{hw}.npz")
    np.savez_compressed(path, **arrays)
    with open(os.path.join(GOLDEN, f"golden_hw{hw}.json"), "w") as f:
        json.dump(summary, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")
