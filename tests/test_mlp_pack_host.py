"""The operand image of the split-precision MLP kernels, read back in MFMA order (no GPU).

`mlp_pack_f16x3` lays the weights out for v_mfma_f32_16x16x32_f16.  This file restates the instruction's lane maps on
their own - lane l = (r = l % 16, g = l // 16); A: row r, k = 8g..8g+7; B: point r, the same k; D: acc[j] = channel 4g + j
of point r - derives from them which hidden channel a k-slot of the next layer holds (two D tiles of a lane ARE its eight
k-slots), and checks that reading the image back through those maps reproduces f16(scale * W) and its residual for every
(layer, cout, cin), each exactly once, including the two-term slots of the raw inputs ([W_hi | W_hi], [W_lo | 0]).
"""
import ctypes as C

import numpy as np
import pytest

from icon_amd import _lib

KIB = 1024
IMAGE_BYTES = 680 * KIB
SIDE_FLOATS = 1060


def chunk_offset_kib(k):
    # [W0 32][layer-1 chunks 0..15: 32 each][chunk 16: 40 = 2 hidden k-steps + 8 raw-input tiles][17..19: 32 each]
    return 32 + 32 * k + (8 if k > 16 else 0)


def channel_of_kslot():
    """k-slot -> channel (0..31) of the 32 hidden channels a K = 32 step covers, from the D and B lane maps alone."""
    out = np.full(32, -1)
    for g in range(4):
        for tile in range(2):           # Ta, Tb: channels 16 * tile + (4g + j) sit in acc[j] of lane group g
            for j in range(4):
                out[8 * g + 4 * tile + j] = 16 * tile + 4 * g + j      # the lane's registers in order = its k-slots 8g..8g+7
    assert sorted(out) == list(range(32))
    return out


def pack(c0, W, B):
    img = np.zeros(IMAGE_BYTES // 2, np.uint16)
    side = np.zeros(SIDE_FLOATS, np.float32)
    inv = np.zeros(3, np.float32)
    scales = np.zeros(5, np.float32)
    pw = (C.c_void_p * 4)(*[w.ctypes.data for w in W])
    pb = (C.c_void_p * 4)(*[b.ctypes.data for b in B])
    _lib.check(_lib.lib().icon_debug_mlp_pack_f16x3(C.c_int(c0), pw, pb, _lib.ptr(img), _lib.ptr(side), _lib.ptr(inv), _lib.ptr(scales)),
               "icon_debug_mlp_pack_f16x3")
    return img.view(np.float16).astype(np.float32), side, inv, scales


def split(ws):
    hi = ws.astype(np.float16).astype(np.float32)
    lo = (ws - hi).astype(np.float16).astype(np.float32)
    return hi, lo


def hidden_tile(img, kib, slot):
    """A operand of one hidden tile as [row r][k]: slot = [64 lanes][8 halves], lane (r, g) holds k = 8g + e."""
    v = img[(kib * KIB + slot * KIB) // 2:][:512].reshape(4, 16, 8)       # [g][r][e]
    return v.transpose(1, 0, 2).reshape(16, 32)


def raw_tile(img, side, kib, tile):
    """The two packed operands the kernel builds from a raw-input tile: a1 = lanes read W_hi at lane & 31, a2 = lanes g < 2
    read W_lo at lane & 31, lanes g >= 2 read the 16 zero bytes of the side arrays."""
    base = (kib * KIB + tile * KIB) // 2
    hi, lo = img[base:base + 256].reshape(32, 8), img[base + 256:base + 512].reshape(32, 8)
    zeros = side[1056:1060]
    assert zeros.tobytes() == bytes(16)
    a1 = np.stack([hi[l & 31] for l in range(64)]).reshape(4, 16, 8).transpose(1, 0, 2).reshape(16, 32)
    a2 = np.stack([lo[l & 31] if l < 32 else np.zeros(8, np.float32) for l in range(64)]).reshape(4, 16, 8).transpose(1, 0, 2).reshape(16, 32)
    return a1, a2


@pytest.mark.parametrize("c0", [7, 13, 16])
def test_image_read_back_in_mfma_order(c0):
    rng = np.random.default_rng(100 + c0)
    cin = [c0, 512, 256 + c0, 128 + c0]
    cout = [512, 256, 128, 1]
    W = [np.ascontiguousarray(rng.standard_normal((co, ci)).astype(np.float32) / np.float32(np.sqrt(ci))) for co, ci in zip(cout, cin)]
    B = [np.ascontiguousarray(rng.standard_normal(co).astype(np.float32) * np.float32(0.1)) for co in cout]
    img, side, inv, scales = pack(c0, W, B)
    s0, s1, s2, A0, A1 = (np.float32(v) for v in scales)
    for v in scales:                                   # powers of two
        assert v > 0 and np.frexp(v)[0] == 0.5
    np.testing.assert_array_equal(inv, np.array([A0 / s0, A1 / s1, np.float32(1) / s2], np.float32))
    chan = channel_of_kslot()

    # layer 0: 32 raw-input tiles in the W0 region
    hi0, lo0 = split(W[0] * s0)
    for ct in range(32):
        a1, a2 = raw_tile(img, side, 0, ct)
        want_hi = np.zeros((16, 16), np.float32); want_lo = np.zeros((16, 16), np.float32)
        want_hi[:, :c0] = hi0[16 * ct:16 * ct + 16]; want_lo[:, :c0] = lo0[16 * ct:16 * ct + 16]
        np.testing.assert_array_equal(a1, np.concatenate([want_hi, want_hi], 1), err_msg=f"layer 0 tile {ct} [W_hi | W_hi]")
        np.testing.assert_array_equal(a2, np.concatenate([want_lo, np.zeros((16, 16), np.float32)], 1), err_msg=f"layer 0 tile {ct} [W_lo | 0]")

    # layer 1: chunk c = k-step c, tile m: hi in slot 2m, lo in 2m + 1
    hi1, lo1 = split((W[1] / A0) * s1)
    rec_hi = np.full((256, 512), np.nan, np.float32); rec_lo = rec_hi.copy(); seen = np.zeros((256, 512), int)
    for c in range(16):
        for m in range(16):
            cols = 32 * c + chan
            rec_hi[16 * m:16 * m + 16, cols] = hidden_tile(img, chunk_offset_kib(c), 2 * m)
            rec_lo[16 * m:16 * m + 16, cols] = hidden_tile(img, chunk_offset_kib(c), 2 * m + 1)
            seen[16 * m:16 * m + 16, cols] += 1
    assert (seen == 1).all()
    np.testing.assert_array_equal(rec_hi, hi1)
    np.testing.assert_array_equal(rec_lo, lo1)

    # layer 2: chunk 16 + q = k-steps 2q, 2q + 1, tile m2 of k-step mm: slot (8 mm + m2) * 2; raw inputs behind chunk 16's k-steps
    W2 = W[2].copy()
    W2[:, :256] = W2[:, :256] / A1
    hi2, lo2 = split(W2 * s2)
    rec_hi = np.full((128, 256), np.nan, np.float32); rec_lo = rec_hi.copy(); seen = np.zeros((128, 256), int)
    for q in range(4):
        for mm in range(2):
            for m2 in range(8):
                cols = 32 * (2 * q + mm) + chan
                rec_hi[16 * m2:16 * m2 + 16, cols] = hidden_tile(img, chunk_offset_kib(16 + q), (8 * mm + m2) * 2)
                rec_lo[16 * m2:16 * m2 + 16, cols] = hidden_tile(img, chunk_offset_kib(16 + q), (8 * mm + m2) * 2 + 1)
                seen[16 * m2:16 * m2 + 16, cols] += 1
    assert (seen == 1).all()
    np.testing.assert_array_equal(rec_hi, hi2[:, :256])
    np.testing.assert_array_equal(rec_lo, lo2[:, :256])
    for m2 in range(8):
        a1, a2 = raw_tile(img, side, chunk_offset_kib(16) + 32, m2)
        want_hi = np.zeros((16, 16), np.float32); want_lo = np.zeros((16, 16), np.float32)
        want_hi[:, :c0] = hi2[16 * m2:16 * m2 + 16, 256:]; want_lo[:, :c0] = lo2[16 * m2:16 * m2 + 16, 256:]
        np.testing.assert_array_equal(a1, np.concatenate([want_hi, want_hi], 1), err_msg=f"layer 2 raw tile {m2}")
        np.testing.assert_array_equal(a2, np.concatenate([want_lo, np.zeros((16, 16), np.float32)], 1), err_msg=f"layer 2 raw tile {m2}")
    assert chunk_offset_kib(19) + 32 == IMAGE_BYTES // KIB

    # side arrays: biases x weight scale in channel order (a lane reads channels 4g..4g+3 of a tile), layer 3 per lane group
    np.testing.assert_array_equal(side[:512], B[0] * s0)
    np.testing.assert_array_equal(side[512:768], B[1] * s1)
    np.testing.assert_array_equal(side[768:896], B[2] * s2)
    w3 = side[896:1056].reshape(4, 40)
    rec = np.full(128, np.nan, np.float32)
    for g in range(4):
        for m2 in range(8):
            rec[16 * m2 + 4 * g:16 * m2 + 4 * g + 4] = w3[g, 4 * m2:4 * m2 + 4]          # acc2[m2][j] of lane group g
        raw = np.zeros(8, np.float32)
        k = np.arange(8) + 8 * (g & 1)                                                    # lane group g carries inputs 8 (g & 1) + s
        raw[k < c0] = W[3][0, 128 + k[k < c0]]
        np.testing.assert_array_equal(w3[g, 32:40], raw)
    np.testing.assert_array_equal(rec, W[3][0, :128])
