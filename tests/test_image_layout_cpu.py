"""CPU checks of the image buffer's layout (csrc/hgs_common.h hgs_image_carve): which fields the kernels read with wide
loads start on 256-byte boundaries, the zero range is one contiguous run that holds the fields it claims, and the loss
head refuses a tile hint it cannot read as uint4 instead of quietly dropping it."""
import ctypes as C

import pytest

SIZES = [(1920, 1080), (800, 800), (1000, 1000), (7, 5), (1, 1), (17, 33), (3840, 2160)]


def _tiles(W, H):
    return ((W + 15) // 16) * ((H + 15) // 16)


def _slots(T):
    n = 64
    while n < T:
        n *= 2
    return n


@pytest.mark.parametrize("W,H", SIZES)
def test_image_fields_start_on_256_byte_boundaries(W, H):
    import hgs_runtime as rt
    lay = rt.layout("image", W, H)
    T = _tiles(W, H)
    # tile_cursor is pinned right behind tile_delta's even number of row-run marks (32-bit atomics only); every other
    # field -- tile_maxc (read as uint4 by the loss head's list builder), status (one 16-byte load per blend workgroup) --
    # starts on a 256-byte boundary
    for name, off in lay.items():
        if name == "tile_cursor":
            assert off % 4 == 0 and off == lay["tile_count"] + 4 * (_slots(T) + ((T + 2) & ~1)), (W, H)
        else:
            assert off % 256 == 0, (name, W, H, off)


@pytest.mark.parametrize("W,H", SIZES)
def test_image_zero_range_is_contiguous_and_covers_the_counters(W, H):
    import hgs_runtime as rt
    L = rt.lib()
    lay = rt.layout("image", W, H)
    T = _tiles(W, H)
    off, nbytes = C.c_size_t(0), C.c_size_t(0)
    rt.check(L.hgs_image_zero_range(W, H, C.addressof(off), C.addressof(nbytes)))
    start, end = off.value, off.value + nbytes.value
    assert start == lay["tile_count"] and nbytes.value % 256 == 0
    # tile_count, tile_delta, tile_cursor, tile_maxc, tile_done, status, tile_prog, tile_sortprog -- in this order, inside
    assert start < lay["tile_cursor"] < lay["tile_maxc"] < lay["status"] < end
    assert lay["tile_maxc"] >= lay["tile_cursor"] + 4 * _slots(T)
    assert lay["status"] >= lay["tile_maxc"] + 2 * 4 * T                 # tile_maxc, tile_done
    assert end >= lay["status"] + 4 * 16 + 2 * 8 * T                      # status words, tile_prog, tile_sortprog (64-bit)
    # behind the range: sort_items (T words), then the blend work list; the buffer holds all of it
    assert end + 4 * T <= lay["tile_order"] < L.hgs_image_bytes(W, H)


def test_misaligned_tile_hint_is_an_error():
    """hgs_loss_head_forward checks the hint before it launches anything: a pointer 8 bytes off a 16-byte boundary (what
    round 6's layout handed it at 1920 x 1080) is refused with a message naming the requirement."""
    import hgs_runtime as rt
    from arguments import OptimizationParams
    from hgs_runtime.strand_step import head_params
    L = rt.lib()
    W, H = 1920, 1080
    hp = head_params(H, W, OptimizationParams(), 0, 0, 1e-6, True)
    hp.tiles_x, hp.tiles_y = (W + 15) // 16, (H + 15) // 16
    fake = 1 << 20                      # (never dereferenced: the call fails on its arguments)
    hp.tile_used = fake + 8
    rc = L.hgs_loss_head_forward(None, C.byref(hp), fake, fake, fake, fake, None, None, fake, fake, None, None)
    assert rc != 0
    msg = L.hgs_last_error().decode()
    assert "tile_used" in msg and "16-byte aligned" in msg, msg
