#!/usr/bin/env python3
"""Leaf-batch flush counts of one cold frame per (scene, camera), from the RT_DIAG build
(rt_debug_phases): flushes, 64-test iterations, guard tests, node visits, and the mid-walk
flushes by the remainder they carried to the next flush.

A cold frame (the first of a fresh scene) runs one wave per 8x8 packet — no heavy-tile split —
so a frame makes packets x (1 + lights) traversals.

usage: CENG795_LIB=diag python tools/leaf_carry.py <scene.xml>[:camera] ...   (one JSON list)
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLUSHES, FLUSH_ITERS, VISITS, EVENTS = 8, 9, 0, 10  # rt_internal.h kPh*
WAVES, CARRY = 30, 31                               # kPhWaves, kPhCarryZero .. kPhCarryHigh


def main():
    if "diag" not in os.environ.get("CENG795_LIB", ""):
        raise SystemExit("run with CENG795_LIB=diag (an RT_DIAG build)")
    import torch
    import ceng795_amd
    from ceng795_amd._lib import lib
    buf = (C.c_ulonglong * 64)()
    out = []
    for arg in sys.argv[1:]:
        xml, _, cam = arg.partition(":")
        cam = int(cam or 0)
        with ceng795_amd.Scene(xml, device=0) as s:
            c = s.camera(cam)
            lib().rt_debug_phases(buf, 64)
            s.debug_counters()
            frame = torch.empty((c.height, c.width, 3), device="cuda")
            s.render_device(cam, frame.data_ptr(),
                            stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            n =lib().rt_debug_phases(buf, 64)
            d = s.debug_counters()
            lights = s.num_lights
        if n < CARRY + 3 or not d["diag_build"]:
            raise SystemExit("not a diagnostic build")
        v = list(buf)[:n]
        packets = ((c.width + 7) // 8) * ((c.height + 7) // 8)
        out.append({"scene": os.path.basename(xml), "camera": cam, "packets": packets,
                    "lights": lights, "waves": v[WAVES], "traversals": packets * (1 + lights),
                    "visits": [v[VISITS], v[EVENTS + VISITS]],
                    "flushes": [v[FLUSHES], v[EVENTS + FLUSHES]],
                    "flush_iters": [v[FLUSH_ITERS], v[EVENTS + FLUSH_ITERS]],
                    "guard_tests": d["guard_tests"],
                    "carry": {"zero": v[CARRY], "low_1_16": v[CARRY + 1],
                              "high_48_63": v[CARRY + 2]}})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
