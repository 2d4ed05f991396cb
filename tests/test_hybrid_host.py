"""The hybrid render's host arithmetic (chroma_amd.gpu.render): pixel packing, the lookup launch schedule, the deterministic
accumulation rule of the lookup tables, the image update and the PNG writer.  No GPU needed."""
import struct
import zlib

import numpy as np

from chroma_amd.gpu.render import (HYBRID_COLORS, hybrid_accumulate, hybrid_chunks, hybrid_image_update, hybrid_pixels,
                                   png_bytes)

f32 = np.float32


def test_pixels_clamp_floor_and_alpha():
    image = np.array([[0.0, 0.5, 1.0], [-1.0, 2.0, 0.999], [np.nan, -0.0, 0.25], [1.0 / 255, 0.004, 1.0 - 1e-7]], f32)
    px = hybrid_pixels(image, 1)
    assert px.dtype == np.uint32
    assert (px >> 24 == 0xFF).all()
    r, g, b = (px >> 16) & 0xFF, (px >> 8) & 0xFF, px & 0xFF
    assert list(r) == [0, 0, 0, 1] and list(g) == [127, 255, 0, 1] and list(b) == [255, 254, 63, 254]
    # the division by nimages comes first, in f32
    two = hybrid_pixels(image * f32(2), 2)
    assert np.array_equal(two, px)
    assert hybrid_pixels(np.array([[3.0, 3.0, 3.0]], f32), 3)[0] == 0xFFFFFFFF


def test_chunk_schedule():
    assert hybrid_chunks(10, 4) == [(4, 10, 0), (4, 10, 4), (4, 10, 8)]
    assert hybrid_chunks(8, 4) == [(4, 8, 0), (4, 8, 4), (4, 8, 8)]            # camera.py: the last launch is wholly past the end
    assert hybrid_chunks(3, 480000) == [(480000, 3, 0)]
    assert [c for _, c in HYBRID_COLORS] == [(1, 0, 0), (0, 1, 0), (0, 0, 1)]


def _loop_accumulate(l1, l2, tri, side, contrib):
    """The rule as a plain loop: per (triangle, side) key, the f32 sum of its records in sample order, added once."""
    sums = {}
    for k in range(len(tri)):
        if tri[k] < 0:
            continue
        key = (int(tri[k]), int(side[k]))
        sums[key] = contrib[k].copy() if key not in sums else (sums[key] + contrib[k]).astype(f32)
    for (t, s), v in sorted(sums.items()):
        table = l1 if s == 1 else l2
        table[t] = (table[t] + v).astype(f32)
    return l1, l2


def test_accumulation_sums_in_sample_order_then_adds_once():
    l1 = np.full((3, 3), 0.5, f32)
    l2 = np.zeros((3, 3), f32)
    tri = np.array([1, 1, 1, -1, 1, 2])
    side = np.array([1, 1, 1, 1, 0, 0])
    c = np.array([[1.0, 0, 0], [1e8, 0, 0], [-1e8, 0, 0], [5, 5, 5], [2, 0, 0], [0, 0, 3]], f32)
    hybrid_accumulate(l1, l2, tri, side, c)
    # 1 + 1e8 rounds to 1e8 in f32, then - 1e8 gives 0: the sum is 0, added once to 0.5
    assert l1[1, 0] == f32(0.5) and l1[0, 0] == f32(0.5) and l1[2, 0] == f32(0.5)
    assert l2[1, 0] == f32(2) and l2[2, 2] == f32(3) and l2[0].sum() == 0
    # a record at a time would have given 0.5 + 1 + 1e8 - 1e8 = 0 (different bits): the rule is not that
    seq = f32(0.5)
    for v in (1.0, 1e8, -1e8):
        seq = f32(seq + f32(v))
    assert seq != l1[1, 0]


def test_accumulation_matches_the_loop_restatement():
    rng = np.random.default_rng(3)
    n, ntri = 5000, 40
    tri = np.where(rng.random(n) < 0.3, -1, rng.integers(0, ntri, n))
    side = rng.integers(0, 2, n)
    c = (rng.random((n, 3)) * rng.choice([1e-3, 1.0, 1e3], (n, 1))).astype(f32)
    base1, base2 = rng.random((ntri, 3)).astype(f32), rng.random((ntri, 3)).astype(f32)
    a1, a2 = hybrid_accumulate(base1.copy(), base2.copy(), tri, side, c)
    b1, b2 = _loop_accumulate(base1.copy(), base2.copy(), tri, side, c)
    assert np.array_equal(a1.view(np.uint32), b1.view(np.uint32)) and np.array_equal(a2.view(np.uint32), b2.view(np.uint32))


def test_image_update():
    l1 = np.array([[1, 2, 3], [4, 5, 6]], f32)
    l2 = np.array([[7, 8, 9], [10, 11, 12]], f32)
    image = np.ones((3, 3), f32)
    hybrid_image_update(image, np.array([1, -1, 0]), np.array([0, 1, 1]), l1, l2, (0, 1, 0), 3)
    assert np.array_equal(image[0], np.array([1, 1 + f32(11) / f32(3), 1], f32))
    assert np.array_equal(image[1], np.ones(3, f32)) and np.array_equal(image[2], np.array([1, 1 + f32(2) / f32(3), 1], f32))


def test_png_round_trip():
    w, h = 7, 5
    rng = np.random.default_rng(1)
    pixels = (rng.integers(0, 1 << 24, w * h).astype(np.uint32) | np.uint32(0xFF000000))
    data = png_bytes(pixels, w, h)
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, chunks = 8, []
    while pos < len(data):
        (length,) = struct.unpack('>I', data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + length]
        assert struct.unpack('>I', data[pos + 8 + length:pos + 12 + length])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        chunks.append((kind, body))
        pos += 12 + length
    assert [k for k, _ in chunks] == [b'IHDR', b'IDAT', b'IEND']
    assert struct.unpack('>IIBBBBB', chunks[0][1]) == (w, h, 8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + 3 * w)
    assert (raw[:, 0] == 0).all()
    rgb = raw[:, 1:].reshape(h, w, 3).astype(np.uint32)
    back = np.uint32(0xFF000000) | rgb[..., 0] << 16 | rgb[..., 1] << 8 | rgb[..., 2]        # row y, column x
    assert np.array_equal(back, pixels.reshape(w, h).T)                                       # ray x * h + y is column x, row y
