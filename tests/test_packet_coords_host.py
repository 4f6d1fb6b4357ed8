"""The frame kernel's packet index arithmetic on the CPU (rt_internal.h: div_magic / div_by,
packet_sel, sel_tile, order_slot — `__host__ __device__`, so rt_host_packet_div and
rt_host_packet_coords run exactly what a wave runs).

A wave divides by wave-uniform values known only at launch (tiles_x, the block-row length, the
number of order regions).  The host turns each divisor d into a multiplier and a shift,
q = (n * mul) >> k with k = 31 + ceil(log2 d) and mul = ceil(2^k / d), which is exact for every
0 <= n < 2^31 (the argument is in rt_internal.h).  Here it is compared with Python's // and %,
no tolerance:

  * for the divisors 1, 2, 3, 5, 7, 8, 15, 16, 17, 240, 241, 480 and 2^k - 1, 2^k, 2^k + 1 up to
    2^28 (tiles_x of the widest frame an int width allows), every dividend below 2^22 (the tiles
    of a 16384 x 16384 frame; C4 has 129,600) and windows of 4096 dividends below and above
    every power of two and every multiple of the divisor nearest to one, up to 2^31 - 1: the
    API sets no smaller limit on a frame's tile count than the int range, and a run over all 2^31
    dividends per divisor does not fit a test;
  * for the launches tests/test_packet_coords_gpu.py renders (and C3's and C4's own frames): each
    logical packet's selected tile, its tile column and row, and the order-list word a
    workgroup reads, against the formulas written with // and %.
"""

import numpy as np
import pytest

from ceng795_amd import _lib, dist_tiles

TRACE_WAVES, BLOCK_W, BLOCK_H = 2, 2, 1  # rt_internal.h kTraceWaves, kBlockW, kBlockH
EXHAUSTIVE = 1 << 22
TOP = (1 << 31) - 1
WINDOW = 4096

DIVISORS = sorted({1, 2, 3, 5, 7, 8, 15, 16, 17, 240, 241, 480} |
                  {d for k in range(1, 29) for d in ((1 << k) - 1, 1 << k, (1 << k) + 1)
                   if 1 <= d <= (1 << 28)})


def quotients(divisor, first, count):
    out = np.empty(count, np.int32)
    rc = _lib.lib().rt_host_packet_div(divisor, first, count, out.ctypes.data)
    assert rc == 0, _lib.lib().rt_last_error().decode()
    return out.astype(np.int64)


def check_range(d, first, count):
    first = max(0, min(first, TOP + 1 - count))
    n = np.arange(first, first + count, dtype=np.int64)
    q = quotients(d, first, count)
    assert np.array_equal(q, n // d), (d, first)
    assert np.array_equal(n - q * d, n % d), (d, first)


@pytest.mark.parametrize("d", DIVISORS)
def test_division_equals_python(d):
    check_range(d, 0, EXHAUSTIVE)
    for k in range(22, 32):
        edge = min(1 << k, TOP)
        check_range(d, edge - WINDOW, 2 * WINDOW)
        check_range(d, (edge // d) * d - WINDOW, 2 * WINDOW)


def test_bad_arguments_are_refused():
    out = np.empty(4, np.int32)
    L = _lib.lib()
    assert L.rt_host_packet_div(0, 0, 4, out.ctypes.data) < 0
    assert L.rt_host_packet_div(3, -1, 4, out.ctypes.data) < 0
    assert L.rt_host_packet_div(3, TOP, 4, out.ctypes.data) < 0
    assert L.rt_host_packet_coords(0, 1, 0, 1, 0, 1, 1, 1, out.ctypes.data) < 0


def model(tiles_x, tiles_y, begin, step, deal, regions, stride, count):
    """(packets, rows of (sel, tx, ty, order word)) of rt_api.hip make_params + rt_kernels.hip
    dispatch_sel / packet_pixel, written with // and %."""
    units = ((tiles_x + 1) // 2) * ((tiles_y + 1) // 2) if deal else tiles_x * tiles_y
    sel_units = (units - begin + step - 1) // step if begin < units else 0
    num_sel = 4 * sel_units if deal else sel_units
    tile_block = step == 1 and not deal and begin % tiles_x == 0 and num_sel % tiles_x == 0
    sel_rows = num_sel // tiles_x
    nbx = (tiles_x + BLOCK_W - 1) // BLOCK_W
    packets = nbx * ((sel_rows + BLOCK_H - 1) // BLOCK_H) * TRACE_WAVES if tile_block else num_sel
    rows = []
    for p in range(count):
        sel = -1
        if p < packets:
            if tile_block:
                w, b = p % TRACE_WAVES, p // TRACE_WAVES
                tx = (b % nbx) * BLOCK_W + w % BLOCK_W
                ty = (b // nbx) * BLOCK_H + w // BLOCK_W
                sel = ty * tiles_x + tx if tx < tiles_x and ty < sel_rows else -1
            else:
                sel = p
        if sel >= num_sel:
            sel = -1
        tx = ty = -1
        if sel >= 0 and deal:
            tx, ty = dist_tiles.deal_block_tile(tiles_x, begin + (sel >> 2) * step, sel & 3)
        elif sel >= 0:
            tile = begin + sel * step
            tx, ty = tile % tiles_x, tile // tiles_x
        rows.append((sel, tx, ty, (p % regions) * stride + p // regions))
    return num_sel, packets, rows


def frame_tiles(width, height, row0=0, row_stride=1):
    rows = (height - row0 + row_stride - 1) // row_stride if row0 < height else 0
    return (width + 7) // 8, (rows + 7) // 8


# every (size, row subset, tile range, deal) of tests/test_packet_coords_gpu.py
SIZES = [(1, 1), (8, 8), (9, 7), (17, 23), (64, 40), (136, 72), (32, 16)]
ROW_SUBSETS = [(0, 1), (2, 1), (0, 3), (2, 3)]
RANGES = [(0, 1), (1, 3), (2, 4), (0, 2)]
LAUNCHES = sorted({(*frame_tiles(w, h, r0, rs), b, s, deal)
                   for w, h in SIZES for r0, rs in ROW_SUBSETS for b, s in RANGES
                   for deal in (0, 1)
                   if ((r0, rs) == (0, 1) or ((b, s) == (0, 1) and not deal)) and r0 < h} |
                  # the benchmark's frames, whole and as a band of tile rows 40 .. 49
                  {(240, 135, 0, 1, 0), (480, 270, 0, 1, 0), (240, 50, 40 * 240, 1, 0),
                   (241, 135, 0, 1, 0), (240, 135, 3, 8, 0), (240, 135, 1, 8, 1)})


@pytest.mark.parametrize("tiles_x,tiles_y,begin,step,deal", LAUNCHES)
@pytest.mark.parametrize("regions", [1, 8, 7])
def test_packet_coordinates_equal_python(tiles_x, tiles_y, begin, step, deal, regions):
    stride = 37
    # (a band: rows tile_begin / tiles_x .. of a taller frame; the kernel sees only the selection)
    full_y = tiles_y + begin // tiles_x if begin and begin % tiles_x == 0 and step == 1 else tiles_y
    num_sel, packets, rows = model(tiles_x, full_y, begin, step, deal, regions, stride, 0)
    count = packets + 2 * TRACE_WAVES + 3  # past the end: no tile
    _, _, rows = model(tiles_x, full_y, begin, step, deal, regions, stride, count)
    out = np.full((count, 4), -9, np.int32)
    got = _lib.lib().rt_host_packet_coords(tiles_x, num_sel, begin, step, deal, regions, stride,
                                           count, out.ctypes.data)
    assert got == packets, _lib.lib().rt_last_error().decode()
    assert out.tolist() == [list(r) for r in rows]
    taken = sorted(r[0] for r in rows if r[0] >= 0)
    assert taken == list(range(num_sel))  # every selected tile, once
