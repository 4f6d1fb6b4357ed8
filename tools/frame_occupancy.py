#!/usr/bin/env python3
"""The HIP runtime's occupancy query for the frame kernel's C3 instantiation
(rt_debug_frame_occupancy): workgroups and waves per CU, static LDS per workgroup, VGPRs.

usage: python tools/frame_occupancy.py [device]   (prints one JSON object)
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from ceng795_amd._lib import check, lib
    out = (C.c_int * 4)()
    check(lib().rt_debug_frame_occupancy(int(sys.argv[1]) if len(sys.argv) > 1 else 0, out))
    print(json.dumps(dict(zip(["workgroups_per_cu", "waves_per_cu", "lds_bytes_per_workgroup",
                               "vgprs"], list(out)))))


if __name__ == "__main__":
    main()
