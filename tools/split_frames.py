#!/usr/bin/env python3
"""Consecutive frames of one camera on one stream from the RT_DIAG build, each frame kept with
the number of waves that rendered it (rt_debug_phases), so a caller can compare with a reference
the very frames whose heavy tiles ran as quadrant waves: the first frame of a
fresh scene is cold, one wave per 8x8 packet; a later one that split tiles has more.

usage: CENG795_LIB=diag python tools/split_frames.py <outdir> <scene.xml>:<camera>:<frames> ...
       writes <outdir>/<argument index>_<frame>.npy (float32 h x w x 3) and prints one JSON list:
       per argument {"camera", "packets", "waves": [per frame], "ray counts": [per frame]}
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WAVES = 30  # rt_internal.h kPhWaves


def main():
    if "diag" not in os.environ.get("CENG795_LIB", ""):
        raise SystemExit("run with CENG795_LIB=diag (an RT_DIAG build)")
    import torch
    import ceng795_amd
    from ceng795_amd._lib import lib
    outdir = sys.argv[1]
    buf = (C.c_ulonglong * 64)()
    out = []
    for k, arg in enumerate(sys.argv[2:]):
        xml, cam, frames = arg.rsplit(":", 2)
        cam, frames = int(cam), int(frames)
        waves, counts = [], []
        with ceng795_amd.Scene(xml, device=0) as s:
            c = s.camera(cam)
            frame = torch.empty((c.height, c.width, 3), device="cuda")
            stream = torch.cuda.current_stream().cuda_stream
            s.collect_stats()
            for f in range(frames):
                frame.fill_(-1.0)
                torch.cuda.synchronize()
                lib().rt_debug_phases(buf, 64)  # (reading clears)
                s.render_device(cam, frame.data_ptr(), stream=stream)
                torch.cuda.synchronize()
                if lib().rt_debug_phases(buf, 64) <= WAVES:
                    raise SystemExit("not a diagnostic build")
                waves.append(int(buf[WAVES]))
                st = s.collect_stats()
                counts.append([st.primary_rays, st.primary_hits, st.shadow_rays])
                np.save(os.path.join(outdir, f"{k}_{f}.npy"), frame.cpu().numpy())
        out.append({"camera": cam, "packets": ((c.width + 7) // 8) * ((c.height + 7) // 8),
                    "waves": waves, "ray counts": counts})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
