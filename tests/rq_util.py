"""Helpers of the ray-query tests: scenes with a camera rig, the oracle's per-ray records as
ray batches, and a tree deeper than the per-lane traversal stack.

The oracle is OracleScene.primary_records: a camera is only a ray generator, so any origin and
direction can be put to the oracle by adding cameras to a SceneSpec.  (Rays no camera generates
go to OracleScene.intersect_rays / shade_rays: tests/ray_batches.py.)  Below them, the GPU
launch helpers the query test files share."""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np

import desc_xml
import scenes
from scenes import G

RIG_W, RIG_H = 33, 31  # odd: an exactly axis-aligned ray at each centre row and column
RIG_AT = {"soup1": (0.1, 0.2, -2.0), "hf_small": (0.05, 0.3, 0.02), "single_sphere": (0, 0, 0),
          "graze_plane": (0, 1e-3, 0), "single_triangle": (0.1, 0.1, 0.5),
          "deep": (0.3, 0.2, 1.0)}


def rig(at):
    """Six cameras at one point gazing +-x +-y +-z, near plane (-1, 1, -1, 1) at distance 1."""
    cams = []
    for axis in range(3):
        for sign in (1, -1):
            gaze = [0, 0, 0]
            gaze[axis] = sign
            up = (0, 0, 1) if axis == 1 else (0, 1, 0)
            cams.append(G.Camera(tuple(at), tuple(gaze), up, (-1, 1, -1, 1), 1, RIG_W, RIG_H,
                                 f"rig{axis}{'p' if sign > 0 else 'n'}.png"))
    return cams


def deep_scene(n: int = 100):
    """A mesh whose reference BVH peels one triangle per level: triangle k sits at
    2^-k (1, 1, 1) and spans 0.8 * 2^-k, so every midpoint split leaves it alone on one side —
    about n levels, more than the 64-entry per-lane traversal stack."""
    verts, faces = [], []
    for k in range(n):
        s, a = 2.0 ** -k, 0.8 * 2.0 ** -k
        verts += [(s, s, s), (s + a, s, s), (s, s + a, s + a)]
        faces.append(f"{3 * k + 1} {3 * k + 2} {3 * k + 3}")
    cam = G.Camera((0.5, 0.5, 4.0), (0, 0, -1), (0, 1, 0), (-1, 1, -1, 1), 3.5, 64, 64, "deep.png")
    return G.SceneSpec(
        cameras=[cam], ambient=(20, 20, 20), lights=[((1.0, 2.0, 5.0), (200, 200, 200))],
        materials=[G.Material((1, 1, 1), (0.8, 0.6, 0.4), (0.2, 0.2, 0.2), phong=4)],
        vertex_text="\n".join(" ".join(repr(float(x)) for x in v) for v in verts),
        meshes=[(1, "\n".join(faces))])


def far_camera(spec_center, diameter: float, width: int = 48, height: int = 48):
    """A camera 2e5 scene diameters away on +z whose image plane (near distance = its distance)
    lies in the scene and spans 1.2 diameters."""
    dist = 2e5 * diameter
    cx, cy, cz = spec_center
    half = 0.6 * diameter
    return G.Camera((cx, cy, cz + dist), (0, 0, -1), (0, 1, 0), (-half, half, -half, half), dist,
                    width, height, "far.png")


def spec_for(name: str):
    if name == "deep":
        return deep_scene()
    return scenes.CATALOGUE[name][0]()


def write_rigged(name: str, directory: str, extra=()) -> str:
    """`name`'s scene with its own cameras, the rig and `extra` cameras: rq_<name>.xml."""
    tag = f"rq_{name}" + ("_far" if extra else "")
    path = os.path.join(directory, tag + ".xml")
    if not os.path.exists(path):
        spec = spec_for(name)
        spec.cameras = list(spec.cameras) + rig(RIG_AT[name]) + list(extra)
        tmp = path + ".tmp"
        with open(tmp, "w") as f:
            f.write(spec.to_xml())
        os.replace(tmp, path)
    return path


@dataclass
class Batch:
    o: np.ndarray       # (n, 3) float32
    d: np.ndarray       # (n, 3) float32, the oracle's normalised directions
    t: np.ndarray       # (n,) the oracle's Hit_data::t (0 where it missed)
    normal: np.ndarray  # (n, 3)
    hit: np.ndarray     # (n,) bool
    cam: np.ndarray     # (n,) the camera each ray came from

    def __len__(self):
        return len(self.o)

    @property
    def skipped_axis(self):
        """Rays for which the reference's slab test skips an axis (|d_i| < 1e-6)."""
        return (np.abs(self.d) < np.float32(1e-6)).any(axis=1)


def camera_positions(xml: str):
    """Each camera's position as the loader reads it (strtof)."""
    import xml.etree.ElementTree as ET
    cams = ET.parse(xml).getroot().find("Cameras").findall("Camera")
    return [np.array(desc_xml.floats(c.find("Position").text), np.float32) for c in cams]


def oracle_batch(xml: str, cameras=None) -> Batch:
    """All (or the given) cameras' rays concatenated in camera order, with the oracle's answers."""
    from oracle.cpu_ref import OracleScene
    o = OracleScene(xml)
    pos = camera_positions(xml)
    parts = {k: [] for k in ("o", "d", "t", "normal", "hit", "cam")}
    for c in (range(o.num_cameras) if cameras is None else cameras):
        rec = o.primary_records(c).reshape(-1, 8)
        parts["o"].append(np.broadcast_to(pos[c], (len(rec), 3)))
        parts["d"].append(rec[:, 0:3])
        parts["t"].append(rec[:, 3])
        parts["normal"].append(rec[:, 4:7])
        parts["hit"].append(rec[:, 7] == 1.0)
        parts["cam"].append(np.full(len(rec), c, np.int32))
    o.close()
    return Batch(*(np.ascontiguousarray(np.concatenate(parts[k])) for k in
                   ("o", "d", "t", "normal", "hit", "cam")))


def object_list(desc):
    """The description's primitives in object-list order: ('T', i0, i1, i2, material) for mesh
    faces in mesh order then loose triangles, ('S', centre bits x3, radius bits, material)."""
    d, a = desc.d, desc.arrays
    out = []
    base = 0
    for m in range(d.num_meshes):
        for f in range(int(a["mesh_face_count"][m])):
            out.append(("T", *a["mesh_faces"][3 * (base + f):3 * (base + f) + 3].tolist(),
                        int(a["mesh_material"][m])))
        base += int(a["mesh_face_count"][m])
    for t in range(d.num_triangles):
        out.append(("T", *a["triangle_indices"][3 * t:3 * t + 3].tolist(),
                    int(a["triangle_material"][t])))
    for k in range(d.num_spheres):
        c = int(a["sphere_center"][k])
        out.append(("S", *desc.verts[3 * c:3 * c + 3].view(np.uint32).tolist(),
                    int(a["sphere_radius"][k:k + 1].view(np.uint32)[0]),
                    int(a["sphere_material"][k])))
    return out


def dump_leaves(text):
    """The leaf lines of a preorder BVH dump, in DFS order, in object_list's form."""
    out = []
    for ln in text.strip().split("\n"):
        tok = ln.split()
        if tok[0] == "T":
            out.append(("T", *(int(x) for x in tok[1:5])))
        elif tok[0] == "S":
            out.append(("S", *(int(x, 16) for x in tok[1:5]), int(tok[5])))
    return out


def dump_depth(text) -> int:
    """Levels of internal nodes in a preorder BVH dump."""
    depth = best = 0
    pending = []  # children still to come at each open node
    for ln in text.strip().split("\n"):
        if ln[0] == "N":
            depth += 1
            best = max(best, depth)
            pending.append(2)
            continue
        while pending:
            pending[-1] -= 1
            if pending[-1]:
                break
            pending.pop()
            depth -= 1
    return best


def scene_xml(name: str, directory: str) -> str:
    """The XML the ray-query tests use for `name`: with the rig where it has a place for one."""
    return write_rigged(name, directory) if name in RIG_AT else scenes.write(name, directory)


# ---------------------------------------------------------------- GPU launch helpers
INF = np.float32(np.inf)


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def trace(s, o, d, *, reorder=False, n=None, stream=None, pad=0, fill=0xA5):
    """rt_trace_rays_device over the first n rays; the output holds `pad` more slots of `fill`
    bytes.  Returns (hits[n], the pad slots' bytes)."""
    import torch
    import ceng795_amd
    rays = ceng795_amd.pack_rays(o, d)
    n = len(rays) if n is None else n
    dr = to_device(rays) if len(rays) else torch.zeros(32, dtype=torch.uint8, device="cuda")
    out = torch.full(((n + pad) * 32 + 32,), fill, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream() if stream is None else stream
    torch.cuda.synchronize()  # the buffers were filled on the current stream
    with torch.cuda.stream(st):
        s.trace_rays_device(dr.data_ptr(), n, out.data_ptr(), reorder=reorder,
                            stream=st.cuda_stream)
    st.synchronize()
    raw = out.cpu().numpy()
    return raw[:n * 32].view(ceng795_amd.HIT_DTYPE).copy(), raw[n * 32:(n + pad) * 32]


def occlusion(s, o, d, tmax, *, reorder=False, n=None, stream=None, pad=0, fill=0xA5):
    import torch
    import ceng795_amd
    rays = ceng795_amd.pack_rays(o, d, tmax)
    n = len(rays) if n is None else n
    dr = to_device(rays) if len(rays) else torch.zeros(32, dtype=torch.uint8, device="cuda")
    out = torch.full((n + pad + 1,), fill, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream() if stream is None else stream
    torch.cuda.synchronize()  # the buffers were filled on the current stream
    with torch.cuda.stream(st):
        s.occluded_device(dr.data_ptr(), n, out.data_ptr(), reorder=reorder,
                          stream=st.cuda_stream)
    st.synchronize()
    raw = out.cpu().numpy()
    return raw[:n].copy(), raw[n:n + pad]


def same_records(a, b):
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


def shade_device(s, o, d, *, n=None, pad=0, stream=None, **kw):
    """rt_shade_rays_device over the first n rays; the output holds `pad` more slots of 0xA5
    bytes.  Returns (radiance[n], the pad slots' bytes)."""
    import torch
    import ceng795_amd
    rays = ceng795_amd.pack_rays(o, d)
    n = len(rays) if n is None else n
    dr = to_device(rays) if len(rays) else torch.zeros(32, dtype=torch.uint8, device="cuda")
    out = torch.full(((n + pad) * 16 + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream() if stream is None else stream
    torch.cuda.synchronize()  # the buffers were filled on the current stream
    with torch.cuda.stream(st):
        s.shade_rays_device(dr.data_ptr(), n, out.data_ptr(), stream=st.cuda_stream, **kw)
    st.synchronize()
    raw = out.cpu().numpy()
    return raw[:n * 16].view(ceng795_amd.RADIANCE_DTYPE).copy(), raw[n * 16:(n + pad) * 16]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_hits_match(hits, b, what):
    """t and normal bit-equal to the oracle's record, ids >= 0 exactly on its hits; a miss is
    (+inf, -1, -1, -1, 0 0 0)."""
    hit = b.hit
    assert np.array_equal(hits["object"] >= 0, hit), what
    assert np.array_equal(hits["leaf"] >= 0, hit) and np.array_equal(hits["material"] >= 0, hit), what
    assert np.array_equal(bits(hits["t"][hit]), bits(b.t[hit])), what
    assert np.array_equal(bits(hits["normal"][hit]), bits(b.normal[hit])), what
    miss = ~hit
    assert (bits(hits["t"][miss]) == bits(INF)).all(), what
    for f in ("object", "material", "leaf"):
        assert (hits[f][miss] == -1).all(), (what, f)
    assert (bits(hits["normal"][miss]) == 0).all() and (hits["pad"] == 0).all(), what
