"""Every frame and query entry on one working set.

The host entries of a scene used from one thread all take the same pooled context, and the
`_device` entries on one caller stream that stream's working set: buffers whose sizes grow and
shrink from call to call, ray-tree frames shared by the frames and the radiance queries of a
recursive scene, and a result buffer that holds three record sizes.  Whatever ran before, every
call must return exactly the bytes the same call returns as the first one on a fresh Scene."""
import functools

import numpy as np
import pytest

import rq_util
import scenes

pytestmark = pytest.mark.gpu

NAMES = ["render_image", "trace_rays 4097", "occluded 65", "shade_rays 1",
         "shade_rays 4097 reorder"]


@functools.lru_cache(maxsize=None)
def rays_of(xml):
    """Every second ray of the scene's camera, with the oracle's normalised directions."""
    b = rq_util.oracle_batch(xml)
    o, d = b.o[::2], b.d[::2]
    assert len(o) >= 4097 and b.hit[::2][:4097].any() and not b.hit[::2][:4097].all()
    return o, d


def host_calls(xml):
    o, d = rays_of(xml)
    return [lambda s: s.render_image(0)[0],
            lambda s: s.trace_rays(o[:4097], d[:4097]),
            lambda s: s.occluded(o[:65], d[:65], 10.0),
            lambda s: s.shade_rays(o[:1], d[:1]),
            lambda s: s.shade_rays(o[:4097], d[:4097], reorder=True)]


def device_calls(xml):
    import torch
    import ceng795_amd
    o, d = rays_of(xml)

    def render(s, st):
        cam = s.camera(0)
        buf = torch.full((cam.height, cam.width, 3), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # the fill ran on the current stream
        s.render_device(0, buf.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        return buf.cpu().numpy()

    def query(entry, n, record, tmax=None, **kw):
        rays = ceng795_amd.pack_rays(o[:n], d[:n], tmax)

        def run(s, st):
            dr = torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()
            out = torch.full((n * record + 16,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            getattr(s, entry)(dr.data_ptr(), n, out.data_ptr(), stream=st.cuda_stream, **kw)
            st.synchronize()
            got = out.cpu().numpy()
            assert (got[n * record:] == 0xA5).all(), entry  # nothing past the n records
            return got
        return run

    return [render,
            query("trace_rays_device", 4097, ceng795_amd.HIT_DTYPE.itemsize),
            query("occluded_device", 65, 1, tmax=10.0),
            query("shade_rays_device", 1, ceng795_amd.RADIANCE_DTYPE.itemsize),
            query("shade_rays_device", 4097, ceng795_amd.RADIANCE_DTYPE.itemsize, reorder=True)]


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and \
        np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_host_entries_share_one_context(scene_dir):
    import ceng795_amd
    xml = scenes.write("soup_depth3", scene_dir)
    calls = host_calls(xml)
    want = []
    for call in calls:
        with ceng795_amd.Scene(xml) as fresh:
            want.append(call(fresh))
    with ceng795_amd.Scene(xml) as s:
        for k in list(range(len(calls))) + list(reversed(range(len(calls)))):
            assert same_bytes(calls[k](s), want[k]), NAMES[k]


def test_device_entries_share_one_stream(scene_dir):
    import torch
    import ceng795_amd
    xml = scenes.write("soup_depth3", scene_dir)
    calls = device_calls(xml)
    want = []
    for call in calls:
        with ceng795_amd.Scene(xml) as fresh:
            want.append(call(fresh, torch.cuda.Stream()))
    with ceng795_amd.Scene(xml) as s:
        st = torch.cuda.Stream()
        for k in list(range(len(calls))) + list(reversed(range(len(calls)))):
            assert same_bytes(calls[k](s, st), want[k]), NAMES[k]
        s.release_stream(st.cuda_stream)
