"""Entry cuts on the GPU: the frame kernel starts a tile's primary walk at the
nodes of the camera's host-built table.  Every render mode below must give the oracle's frame (or
records) bit for bit with the table bound (switch 0) and with every walk started at the root
(rt_test_entry_cuts(1), a process-wide switch nothing else sets), and so the same with both."""
import contextlib
import functools

import numpy as np
import pytest

import entry_cut_scenes as ECS
from ceng795_amd import _lib
from oracle.cpu_ref import OracleScene

pytestmark = pytest.mark.gpu

NAMES = ["cut_hf", "cut_ragged", "cut_inside", "cut_far", "cut_axis", "cut_two", "cut_s2m20",
         "cut_t1e5"]


@functools.lru_cache(maxsize=None)
def oracle_frame(xml, cam):
    ref = OracleScene(xml).render(cam, threads=8)[0]
    ref.setflags(write=False)
    return ref


@contextlib.contextmanager
def entry_cuts(mode):
    assert _lib.lib().rt_test_entry_cuts(mode) == 0
    try:
        yield
    finally:
        assert _lib.lib().rt_test_entry_cuts(0) == 0


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def render_modes(s, cam, ref):
    """Every mode's output for camera `cam`, by name; each checked against the oracle's frame."""
    import torch
    h, w, _ = ref.shape
    out = {}
    st = torch.cuda.Stream()

    def fresh(shape=None, dtype=torch.float32, fill=-1.0):
        buf = torch.full(shape or ref.shape, fill, dtype=dtype, device="cuda")
        torch.cuda.synchronize()  # the fill ran on the current stream
        return buf

    def host(buf):
        st.synchronize()  # the renders run on `st`
        return buf.cpu().numpy()

    # the whole frame on one stream: cold, then warm frames, which split the heaviest tiles over
    # their workgroup's four waves (as tests/test_gpu_parity.py's split test renders them)
    for k in range(4):
        buf = fresh()
        s.render_device(cam, buf.data_ptr(), stream=st.cuda_stream)
        out[f"frame{k}"] = host(buf)
        assert same(out[f"frame{k}"], ref), k
    # a band from a tile row on (the table is bound from that row), and one from row 4 (it is not)
    for row0 in (8, 4):
        buf = fresh()
        s.render_device(cam, buf.data_ptr(), starting_row=row0, stream=st.cuda_stream)
        got = host(buf)
        out[f"band{row0}"] = got
        assert same(got[row0:], ref[row0:]) and (got[:row0] == -1.0).all(), row0
    # a band of whole tile rows cut out of the frame's tiles
    tiles_x, tiles_y = (w + 7) // 8, (h + 7) // 8
    if tiles_y >= 3:
        buf = fresh()
        s.render_device(cam, buf.data_ptr(), tile_begin=tiles_x, tile_count=tiles_x * (tiles_y - 2),
                        stream=st.cuda_stream)
        got = host(buf)
        out["tile_band"] = got
        y1 = 8 * (tiles_y - 1)
        assert same(got[8:y1], ref[8:y1]) and (got[:8] == -1.0).all() and (got[y1:] == -1.0).all()
    # rows 1, 3, 5, ... through rt_render: strided rows, no table
    img = np.full(ref.shape, -1.0, np.float32)
    s.render_image(cam, img, starting_row=1, height_increase=2)
    out["odd_rows"] = img[1::2]
    assert same(img[1::2], ref[1::2])
    # a 2x2-block tile deal over three ranks, tile-major shares, untiled into one frame
    world = 3
    blocks = ((tiles_x + 1) // 2) * ((tiles_y + 1) // 2)
    slot = 4 * ((blocks + world - 1) // world)
    shares = fresh((world, slot, 64, 3), fill=-3.0)
    for r in range(world):
        s.render_device(cam, shares[r].data_ptr(), tile_begin=r, tile_step=world, tile_major=True,
                        blocks=True, stream=st.cuda_stream)
    buf = fresh()
    s.untile_device(cam, world, slot, shares.data_ptr(), buf.data_ptr(), blocks=True,
                    stream=st.cuda_stream)
    out["deal"] = host(buf)
    assert same(out["deal"], ref)
    # pixel records of the whole frame, and the frame shaded from them
    if s.records_ok(cam):
        recs = fresh((h, w), torch.int32, -1)
        s.render_device(cam, recs.data_ptr(), records=True, stream=st.cuda_stream)
        buf = fresh()
        s.resolve_rows(cam, 0, h, recs.data_ptr(), buf.data_ptr(), stream=st.cuda_stream)
        out["records"] = host(recs)
        assert same(host(buf), ref)
    torch.cuda.synchronize()
    s.release_stream(st.cuda_stream)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_every_mode_with_and_without_the_cuts(scene_dir, name):
    import ceng795_amd
    xml = ECS.write(name, scene_dir)
    cams = ECS.SCENES[name][1] or OracleScene(xml).num_cameras
    with ceng795_amd.Scene(xml) as s:
        for cam in range(cams):
            ref = oracle_frame(xml, cam)
            with entry_cuts(0):
                bound = render_modes(s, cam, ref)
            with entry_cuts(1):
                rooted = render_modes(s, cam, ref)
            assert bound.keys() == rooted.keys()
            for mode in bound:
                assert same(bound[mode], rooted[mode]), (name, cam, mode)
