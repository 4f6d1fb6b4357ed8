"""Helpers of the ray-query tests: scenes with a camera rig, the oracle's per-ray records as
ray batches, and a tree deeper than the per-lane traversal stack.

The oracle is OracleScene.primary_records: a camera is only a ray generator, so any origin and
direction can be put to the oracle by adding cameras to a SceneSpec."""
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
