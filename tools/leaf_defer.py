#!/usr/bin/env python3
"""The leaf batch's deferred guard on one cold frame per (scene, camera), from the
RT_DIAG build (rt_debug_phases): per traversal kind (primary, shadow) the queued leaf tests, the
64-test iterations that ran them, the survivors (triangle or sphere test hit in range), the
64-survivor guard iterations, the guard batches that split one iteration's survivors, and the
survivors the guard rejected.

A cold frame (the first of a fresh scene) runs one wave per 8x8 packet — no heavy-tile split —
so a frame makes `packets` primary and `packets x lights` shadow traversals.

usage: CENG795_LIB=diag python tools/leaf_defer.py <scene.xml>[:camera] ...   (one JSON list)
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLUSHES, FLUSH_ITERS, EVENTS = 8, 9, 10  # rt_internal.h kPh*
WAVES, DEFER_PRIM, DEFER_SHAD = 30, 34, 38  # kPhWaves, kPhDeferPrim, kPhDeferShad
NAMES = ["survivors", "guard_iters", "split_drains", "guard_rejected"]  # kDf*


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
            n = lib().rt_debug_phases(buf, 64)
            d = s.debug_counters()
            lights = s.num_lights
        if n < DEFER_SHAD + len(NAMES) or not d["diag_build"]:
            raise SystemExit("not a diagnostic build with the deferred-guard counters")
        v = list(buf)[:n]
        packets = ((c.width + 7) // 8) * ((c.height + 7) // 8)
        kinds = {}
        for kind, ev, at, tests, trav in (
                ("primary", 0, DEFER_PRIM, d["prim_leaf_lanes"], packets),
                ("shadow", EVENTS, DEFER_SHAD, d["shad_leaf_lanes"], packets * lights)):
            kinds[kind] = dict(zip(NAMES, v[at:at + len(NAMES)]), leaf_tests=tests,
                               traversals=trav, flushes=v[ev + FLUSHES],
                               flush_iters=v[ev + FLUSH_ITERS])
        out.append({"scene": os.path.basename(xml), "camera": cam, "packets": packets,
                    "lights": lights, "waves": v[WAVES], "guard_tests": d["guard_tests"], **kinds})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
