#!/usr/bin/env python3
"""The frame kernel's octant loop (rt_kernels.hip octant_walks) on frames of a
fresh scene, from the RT_DIAG build (rt_debug_phases): per frame the waves that ran, and per
traversal kind (primary; shadow, per light) the packets that had an active lane and the sub-walks
they made — one per direction-sign octant among the packet's active lanes.

The first frame of a fresh scene is cold: one wave per 8x8 packet.  Later frames on the same
stream dispatch by the previous frame's costs and may split heavy tiles over four quadrant waves
(DESIGN.md §4.9): `waves` then exceeds the packets.

usage: CENG795_LIB=diag python tools/octant_walks.py <scene.xml>[:camera[:frames]] ...
       (one JSON list; per argument a list of `frames` frames, default 1)
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WAVES, OCT = 30, 42  # rt_internal.h kPhWaves, kPhOctPrimPackets


def main():
    if "diag" not in os.environ.get("CENG795_LIB", ""):
        raise SystemExit("run with CENG795_LIB=diag (an RT_DIAG build)")
    import torch
    import ceng795_amd
    from ceng795_amd._lib import lib
    buf = (C.c_ulonglong * 64)()
    out = []
    for arg in sys.argv[1:]:
        xml, _, rest = arg.partition(":")
        cam, _, frames = rest.partition(":")
        cam, frames = int(cam or 0), int(frames or 1)
        per_frame = []
        with ceng795_amd.Scene(xml, device=0) as s:
            c = s.camera(cam)
            frame = torch.empty((c.height, c.width, 3), device="cuda")
            for _ in range(frames):
                lib().rt_debug_phases(buf, 64)  # (reading clears)
                s.render_device(cam, frame.data_ptr(),
                                stream=torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                n = lib().rt_debug_phases(buf, 64)
                if n < OCT + 4:
                    raise SystemExit("not a diagnostic build with the octant counters")
                v = list(buf)[:n]
                per_frame.append({
                    "packets": ((c.width + 7) // 8) * ((c.height + 7) // 8), "waves": v[WAVES],
                    "primary": {"packets": v[OCT], "walks": v[OCT + 1]},
                    "shadow": {"packets": v[OCT + 2], "walks": v[OCT + 3]}})
        out.append({"scene": os.path.basename(xml), "camera": cam, "frames": per_frame})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
