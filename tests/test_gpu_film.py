"""Films on the GPU (rt_film_*, ceng795_amd.Film): every comparison is bit for bit, on the raw
accumulators and on the resolved frame, against tests/film_util.py's restatement of the contract
(pinned to the oracle's MSAA frame by tests/test_film_host.py), the library's own frames and the
oracle's."""
import ctypes as C
import os

import numpy as np
import pytest

import film_util as FU
import scenes
from conftest import assert_parity
from oracle.cpu_ref import OracleScene
from rq_util import to_device

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
f32 = np.float32


def rt():
    import ceng795_amd
    return ceng795_amd


def check_film(film, acc, what):
    """The film's accumulators and resolved frame against the restated film `acc`."""
    got = film.accumulators()
    differing = int((FU.bits(got) != FU.bits(acc)).sum())
    if differing:
        at = np.argwhere(FU.bits(got) != FU.bits(acc))[0]
        raise AssertionError(f"{what}: {differing} accumulator channels differ, first at "
                             f"(row, column, channel) {tuple(at)}: got {got[tuple(at)]!r}, "
                             f"want {acc[tuple(at)]!r}")
    assert FU.same_bits(film.resolve(), FU.resolve(acc)), f"{what}: resolved frame differs"


def radiance(rgb):
    out = np.zeros(len(rgb), rt().RADIANCE_DTYPE)
    out["rgb"] = rgb
    out["t"] = f32(7)  # ignored
    return out


def device_batch(xy, rgb):
    """(xy, rad) as device tensors (kept alive by the caller) of a splat_device call."""
    return to_device(np.array(xy, f32)), to_device(radiance(rgb))


_ANCHOR = {}


def anchor(scene_dir, name, seed):
    """The MSAA samples of camera 0 and what they must give: computed once per (scene, seed)."""
    key = (name, seed)
    if key not in _ANCHOR:
        xml = scenes.write(name, scene_dir)
        o, d, xy, (w, h, S) = FU.msaa_samples(xml, 0, seed)
        oracle, _ = OracleScene(xml).render_msaa(0, seed=seed, threads=THREADS)
        with rt().Scene(xml) as s:
            s.set_msaa_seed(seed)
            frame, _ = s.render_image(0)
            rad = s.shade_rays(o, d)
        acc = FU.new_film(w, h)
        FU.splat(acc, xy, rad["rgb"])
        for a in (o, d, xy, oracle, frame, rad, acc):
            a.setflags(write=False)
        _ANCHOR[key] = dict(xml=xml, o=o, d=d, xy=xy, w=w, h=h, S=S, oracle=oracle, frame=frame,
                            rad=rad, acc=acc)
    return _ANCHOR[key]


# ---------------------------------------------------------------- 1. the anchor
@pytest.mark.parametrize("name", list(scenes.MSAA))
def test_film_of_the_msaa_samples_is_the_msaa_frame(scene_dir, name):
    """film == the library's own MSAA render_image == OracleScene.render_msaa, through the fused
    entry and through Scene.shade_rays + splat, for two seeds."""
    frames = []
    for seed in (0, 7):
        a = anchor(scene_dir, name, seed)
        frames.append(a["oracle"])
        with rt().Scene(a["xml"]) as s:
            with rt().Film(s, a["w"], a["h"]) as fused, rt().Film(s, a["w"], a["h"]) as two_step:
                st = fused.shade_rays(a["o"], a["d"], a["xy"], stats=True)
                two_step.splat(a["xy"], s.shade_rays(a["o"], a["d"]))
                assert st.primary_rays == len(a["xy"])
                for film, what in ((fused, "fused"), (two_step, "shade_rays + splat")):
                    what = f"{name}/seed{seed}/{what}"
                    check_film(film, a["acc"], what)
                    assert film.counts() == (len(a["xy"]), 0), what
                    got = film.resolve()
                    assert FU.same_bits(got, a["frame"]), f"{what}: not the library's MSAA frame"
                    if name == "msaa9_depth2":
                        assert_parity(got, a["oracle"], what)
                    else:
                        assert FU.same_bits(got, a["oracle"]), f"{what}: not the oracle's frame"
    assert (FU.bits(frames[0]) != FU.bits(frames[1])).any(axis=-1).sum() > 0, "the seeds agree"


# ---------------------------------------------------------------- 2. order
def test_order_across_pixels_is_free_and_within_a_pixel_is_kept(scene_dir):
    a = anchor(scene_dir, "msaa4", 0)
    xy, rgb, w, h, S = a["xy"], a["rad"]["rgb"], a["w"], a["h"], a["S"]
    n = len(xy)
    rng = np.random.default_rng(5)
    pix = FU.source_pixels(xy, w)
    # slot k of the shuffled batch belongs to pixel pix[perm[k]]; each pixel's slots, ascending,
    # take its samples in their original order
    perm = rng.permutation(n)
    order = np.empty(n, np.int64)
    order[np.argsort(pix[perm], kind="stable")] = np.argsort(pix, kind="stable")
    assert not np.array_equal(order, np.arange(n))
    for p in rng.integers(0, w * h, 16):
        mine = order[pix[order] == p]
        assert len(mine) == S and (np.diff(mine) > 0).all()
    # ... and each pixel's samples reversed
    rev = np.arange(n).reshape(-1, S)[:, ::-1].reshape(-1)
    acc_rev = FU.new_film(w, h)
    FU.splat(acc_rev, xy[rev], rgb[rev])
    assert int((FU.bits(acc_rev) != FU.bits(a["acc"])).sum()) >= 100, "the order does not show"
    with rt().Scene(a["xml"]) as s, rt().Film(s, w, h) as film:
        film.splat(xy[order], rgb[order])
        check_film(film, a["acc"], "shuffled across pixels")
        film.clear()
        film.splat(xy[rev], rgb[rev])
        check_film(film, acc_rev, "reversed within pixels")


# ---------------------------------------------------------------- 3. calls
def test_calls_add_in_sequence(scene_dir):
    a = anchor(scene_dir, "msaa5", 7)
    xy, rgb, w, h = a["xy"], a["rad"]["rgb"], a["w"], a["h"]
    n = len(xy)
    with rt().Scene(a["xml"]) as s, rt().Film(s, w, h) as film:
        for row in (1, h // 2, h - 1):  # two calls cut between source rows = one call
            top = np.floor(xy[:, 1]) < row
            film.clear()
            assert film.counts() == (0, 0)
            film.splat(xy[top], rgb[top])
            film.splat(xy[~top], rgb[~top])
            check_film(film, a["acc"], f"cut above row {row}")
        # an index cut of a batch in no pixel order: the restatement, call after call
        perm = np.random.default_rng(9).permutation(n)
        sxy, srgb = xy[perm], rgb[perm]
        for cut in (1, n - 3, 777):
            acc = FU.new_film(w, h)
            film.clear()
            for part in (slice(0, cut), slice(cut, n)):
                FU.splat(acc, sxy[part], srgb[part])
                film.splat(sxy[part], srgb[part])
            check_film(film, acc, f"cut at index {cut}")
            assert film.counts() == (n, 0)
        one = FU.new_film(w, h)
        FU.splat(one, sxy, srgb)
        assert int((FU.bits(acc) != FU.bits(one)).sum()) > 0  # (a cut by index is another order)


# ---------------------------------------------------------------- 4. list lengths
LENGTHS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 257]


def random_batch(rng, width, height, lengths):
    """lengths[p] samples in pixel p at random places of it, random colours, batch order shuffled."""
    pix = np.repeat(np.arange(width * height), lengths)
    rng.shuffle(pix)
    frac = rng.random((len(pix), 2)).astype(f32) * f32(0.999)
    xy = np.stack([(pix % width).astype(f32) + frac[:, 0], (pix // width).astype(f32) + frac[:, 1]], 1)
    rgb = (rng.random((len(pix), 3)) * 300).astype(f32)
    assert np.array_equal(FU.source_pixels(xy, width), pix)
    return xy.astype(f32), rgb


@pytest.mark.parametrize("width,height,lengths,filter,sigma", [
    # every pixel of these films is on an edge; lists of every length beside empty ones
    (5, 4, [0, 1, 0, 2, 31, 32, 0, 33, 0, 63, 64, 0, 65, 0, 257, 0, 0, 1, 0, 0], "gaussian", None),
    (5, 4, [257, 0, 65, 64, 0, 63, 33, 0, 32, 31, 2, 0, 1, 0, 0, 0, 0, 0, 0, 1], "gaussian", 0.5),
    (5, 4, [0, 1, 0, 2, 31, 32, 0, 33, 0, 63, 64, 0, 65, 0, 257, 0, 0, 1, 0, 0], "box", None),
    (1, 1, [257], "gaussian", None),
    (1, 1, [5000], "gaussian", None),      # longer than the sort's LDS buffer
    (3, 2, [65, 0, 33, 1, 257, 2], "gaussian", None),
    (70, 40, None, "gaussian", None),      # more pixels than one scan workgroup takes
    (2049, 2049, None, "gaussian", None),  # ... and than two scan levels take
])
def test_list_lengths(scene_dir, width, height, lengths, filter, sigma):
    rng = np.random.default_rng(width * 131 + height)
    if lengths is None:  # LENGTHS scattered over the film, first and last pixel included
        lengths = np.zeros(width * height, np.int64)
        at = np.concatenate([[0, width * height - 1], rng.integers(0, width * height, 38)])
        lengths[at] = np.resize(LENGTHS[1:], len(at))
    xy, rgb = random_batch(rng, width, height, lengths)
    acc = FU.new_film(width, height)
    assert FU.splat(acc, xy, rgb, filter, sigma) == (len(xy), 0)
    xml = scenes.write("soup1", scene_dir)
    with rt().Scene(xml) as s, rt().Film(s, width, height, filter=filter, sigma=sigma) as film:
        film.splat(xy, rgb)
        check_film(film, acc, f"{width}x{height} {filter} sigma {sigma}")
        assert film.counts() == (len(xy), 0)
        untouched = acc[..., 3] == 0
        if untouched.any():
            assert (FU.bits(film.resolve()[untouched]) == 0).all()  # 0 0 0, not NaN


# ---------------------------------------------------------------- 5. validity
def test_invalid_samples_are_dropped_and_counted(scene_dir):
    w, h = 7, 5
    rng = np.random.default_rng(11)
    n = 192  # three waves
    xy = np.stack([rng.random(n) * w, rng.random(n) * h], 1).astype(f32) * f32(0.999)
    rgb = (rng.random((n, 3)) * 10).astype(f32)
    keep = np.ones(n, bool)
    inf = f32(np.inf)
    edge = np.nextafter(f32(w), f32(0))
    xy[5] = (f32(-0.0), 1.5)     # valid: pixel 0 of its row
    xy[6] = (edge, f32(-0.0))    # valid: the last column, the first row
    xy[7] = (2.5, np.nextafter(f32(h), f32(0)))
    bad = [(f32(w), 1.0), (f32(-1e-30), 1.0), (f32(np.nan), 1.0), (inf, 1.0), (-inf, 1.0),
           (f32(1e30), 1.0), (f32(-1), 1.0), (1.0, f32(h)), (1.0, f32(-1e-30)), (1.0, f32(np.nan)),
           (1.0, -inf), (f32(np.nan), f32(np.nan))]
    slots = [0, 63, 64, 127, 128, 191, 1, 62, 65, 126, 129, 190]  # lanes 0 and 63 of each wave first
    for slot, value in zip(slots, bad):
        xy[slot] = value
        keep[slot] = False
    acc = FU.new_film(w, h)
    FU.splat(acc, xy[keep], rgb[keep], valid=np.ones(int(keep.sum()), bool))
    assert np.array_equal(FU.valid_mask(xy, w, h), keep)  # (the restatement's own rule agrees)
    xml = scenes.write("soup1", scene_dir)
    with rt().Scene(xml) as s, rt().Film(s, w, h) as film:
        film.splat(xy, rgb)
        assert film.counts() == (int(keep.sum()), len(bad))
        check_film(film, acc, "invalid positions")
        film.splat(xy[~keep], rgb[~keep])  # a call of invalid samples only changes nothing
        assert film.counts() == (int(keep.sum()), 2 * len(bad))
        check_film(film, acc, "only invalid positions")


def test_invalid_rays_are_dropped_by_the_fused_entry(scene_dir):
    a = anchor(scene_dir, "msaa4", 0)
    n = 640
    o, d, xy = a["o"][:n].copy(), a["d"][:n].copy(), a["xy"][:n]
    keep = np.ones(n, bool)
    for k, (arr, value) in {0: (o, np.nan), 63: (d, np.inf), 64: (d, 0.0), 200: (o, -np.inf),
                            639: (d, np.nan)}.items():
        arr[k] = value if value == 0.0 else (value, arr[k][1], arr[k][2])
        keep[k] = False
    d[300] = (0.0, 0.0, 1e-7)  # every |d_i| < 1e-6: invalid as well
    keep[300] = False
    with rt().Scene(a["xml"]) as s, rt().Film(s, a["w"], a["h"]) as film, \
            rt().Film(s, a["w"], a["h"]) as want:
        film.shade_rays(o, d, xy)
        want.splat(xy[keep], s.shade_rays(o[keep], d[keep]))
        assert film.counts() == (int(keep.sum()), int((~keep).sum())) == (n - 6, 6)
        check_film(film, want.accumulators(), "invalid rays")


# ---------------------------------------------------------------- 6. box = frame
@pytest.mark.parametrize("name", ["soup1", "soup_depth3"])
def test_box_film_of_pixel_centre_rays_is_the_frame(scene_dir, name):
    xml = scenes.write(name, scene_dir)
    cam = FU.camera(xml, 0)
    o, d, xy = FU.pixel_centre_samples(cam)
    w, h = cam[4], cam[5]
    with rt().Scene(xml) as s, rt().Film(s, w, h, filter="box") as film:
        frame, _ = s.render_image(0)
        film.shade_rays(o, d, xy)
        assert FU.same_bits(film.resolve(), frame), f"{name}: box film != render_image"
        assert (film.accumulators()[..., 3] == 1).all()
        # four samples per pixel, anywhere in it
        rng = np.random.default_rng(3)
        xy4, rgb4 = random_batch(rng, w, h, np.full(w * h, 4))
        acc = FU.new_film(w, h)
        FU.splat(acc, xy4, rgb4, "box")
        film.clear()
        film.splat(xy4, rgb4)
        check_film(film, acc, f"{name}: four box samples per pixel")


# ---------------------------------------------------------------- 7. plumbing
def test_refusals(scene_dir):
    from ceng795_amd import _lib
    L = _lib.lib()
    xml = scenes.write("soup1", scene_dir)
    with rt().Scene(xml) as s:
        h = C.c_void_p()
        for args in ((0, 8, 0, 0.0), (8, 0, 0, 0.0), (32769, 8, 0, 0.0), (8, 32769, 0, 0.0),
                     (-1, 8, 0, 0.0), (8, 8, 2, 0.0), (8, 8, -1, 0.0), (8, 8, 0, -0.5),
                     (8, 8, 0, float("nan")), (8, 8, 0, float("inf"))):
            assert L.rt_film_create(s.handle, *args, C.byref(h)) == _lib.RT_E_INVALID, args
            assert not h.value
        with rt().Film(s, 8, 8) as film:
            buf = np.zeros(64, f32)
            p = buf.ctypes.data + (-buf.ctypes.data % 16)
            P = C.c_void_p
            calls = {"n < 0": lambda: L.rt_film_splat(film.handle, P(p), P(p), -1),
                     "xy misaligned": lambda: L.rt_film_splat(film.handle, P(p + 4), P(p), 1),
                     "rad misaligned": lambda: L.rt_film_splat(film.handle, P(p), P(p + 8), 1),
                     "n too large": lambda: L.rt_film_splat(film.handle, P(p), P(p), (1 << 28) + 1),
                     "device n too large": lambda: L.rt_film_splat_device(film.handle, P(p), P(p),
                                                                           (1 << 28) + 1, None),
                     "rays misaligned": lambda: L.rt_film_shade_rays(film.handle, P(p + 8), P(p), 1,
                                                                     -1, 0, None),
                     "flag": lambda: L.rt_film_shade_rays(film.handle, P(p), P(p), 1, -1, 4, None),
                     "depth": lambda: L.rt_film_shade_rays(film.handle, P(p), P(p), 1, 99, 0, None),
                     "NULL xy": lambda: L.rt_film_splat(film.handle, None, P(p), 1)}
            for what, call in calls.items():
                assert call() == _lib.RT_E_INVALID, what
            assert film.counts() == (0, 0)
    with rt().Scene(xml, devices=[0, 0]) as s:
        with pytest.raises(rt().RTError) as e:
            rt().Film(s, 8, 8)
        assert e.value.code == _lib.RT_E_UNSUPPORTED and "multi-device" in str(e.value)


def test_streams_scratch_and_host_device_entries(scene_dir):
    import torch
    a = anchor(scene_dir, "msaa4", 0)
    xy, rgb, w, h = a["xy"], a["rad"]["rgb"], a["w"], a["h"]
    n = len(xy)
    half = n // 2
    acc_half = FU.new_film(w, h)
    FU.splat(acc_half, xy[:half], rgb[:half])
    acc_two = acc_half.copy()
    FU.splat(acc_two, xy[half:], rgb[half:])
    with rt().Scene(a["xml"]) as s:
        s.set_msaa_seed(0)
        with rt().Film(s, w, h) as f1, rt().Film(s, w, h) as f2:
            for _ in range(12):  # create / destroy
                rt().Film(s, 31, 17, filter="box").close()
            # n = 0 launches nothing, whatever the pointers
            f1.splat_device(0, 0, 0)
            f1.shade_rays_device(0, 0, 0)
            f1.splat(np.zeros((0, 2), f32), np.zeros((0, 3), f32))
            assert f1.counts() == (0, 0) and (FU.bits(f1.accumulators()) == 0).all()
            assert (FU.bits(f1.resolve()) == 0).all()  # untouched pixels resolve to 0
            # two films on two streams, a frame between the two splats of one of them
            d_a, d_b, d_all = (device_batch(xy[:half], rgb[:half]), device_batch(xy[half:], rgb[half:]),
                               device_batch(xy, rgb))
            frame = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
            out1 = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
            s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
            torch.cuda.synchronize()
            f1.splat_device(d_a[0].data_ptr(), d_a[1].data_ptr(), half, stream=s1.cuda_stream)
            f2.splat_device(d_all[0].data_ptr(), d_all[1].data_ptr(), n, stream=s2.cuda_stream)
            s.render_device(0, frame.data_ptr(), stream=s1.cuda_stream)
            f1.splat_device(d_b[0].data_ptr(), d_b[1].data_ptr(), n - half, stream=s1.cuda_stream)
            f1.resolve_device(out1.data_ptr(), stream=s1.cuda_stream)
            torch.cuda.synchronize()
            check_film(f1, acc_two, "two splats around a frame")
            check_film(f2, a["acc"], "the other stream's film")
            assert FU.same_bits(out1.cpu().numpy().reshape(h, w, 3), FU.resolve(acc_two))
            assert FU.same_bits(frame.cpu().numpy().reshape(h, w, 3), a["frame"])
            # the scratch goes and comes back
            s.release_stream(s1.cuda_stream)
            f1.clear_device(stream=s1.cuda_stream)
            f1.splat_device(d_a[0].data_ptr(), d_a[1].data_ptr(), half, stream=s1.cuda_stream)
            s1.synchronize()
            check_film(f1, acc_half, "after rt_release_stream_scratch")
            assert f1.counts() == (half, 0)
            # the fused device entry = the fused host entry
            rays = to_device(rt().pack_rays(a["o"], a["d"]))
            torch.cuda.synchronize()  # (uploaded on the current stream)
            f1.clear_device(stream=s1.cuda_stream)
            f1.shade_rays_device(rays.data_ptr(), d_all[0].data_ptr(), n, stream=s1.cuda_stream)
            s1.synchronize()
            f2.clear()
            f2.shade_rays(a["o"], a["d"], xy)
            check_film(f1, a["acc"], "fused device entry")
            check_film(f2, a["acc"], "fused host entry")
            assert s.collect_stats().primary_rays >= n
