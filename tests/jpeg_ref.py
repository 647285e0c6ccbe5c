"""The Motion-JPEG pipe format restated in integers (numpy only, no torch): the definition in the header comment of csrc/jpeg.hip, which
the device must reproduce byte for byte, plus the two walkers the tests read streams and AVI files with.

    encode(rgb, quality, restart_mcus) -> bytes      one baseline JPEG: 4:2:0, standard Huffman tables, restart intervals
    header(h, w, quality, restart_mcus) -> bytes     SOI .. SOS header (what maua_jpeg_header writes)
    walk(stream) -> dict                             marker walker (segments, DRI, entropy span, RST positions)
    avi_frames(path) -> dict                         RIFF walker (00dc payloads, avih / strh / strf fields, idx1 entries)
"""
import struct

import numpy as np

# ITU-T T.81 Annex K.1 / K.2, natural (row-major) order
QUANT_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
              18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
QUANT_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
# natural index of the k-th coefficient in zig-zag order
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
# ITU-T T.81 Annex K.3: (BITS, HUFFVAL) of the four standard tables
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08,
    0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
    0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
    0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
    0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
    0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
    0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])
HUFF_TABLES = [(0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)]  # (Tc << 4 | Th, table) in stream order

# the 13-bit constants of the integer DCT: round(x * 8192)
F_0_298631336, F_0_390180644, F_0_541196100, F_0_765366865, F_0_899976223, F_1_175875602 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501321110, F_1_847759065, F_1_961570560, F_2_053119869, F_2_562915447, F_3_072711026 = 12299, 15137, 16069, 16819, 20995, 25172
SEGMENT_BYTES_PER_MCU = 2496  # worst case of one MCU's entropy data after stuffing (derivation: csrc/jpeg.hip)


def scaled_tables(quality):
    """The two quantisation tables (natural order, lists of 64 ints) at ``quality`` 1..95, scaled the IJG way."""
    if not 1 <= quality <= 95:
        raise ValueError(f"quality {quality} outside 1..95")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [[min(max((t * scale + 50) // 100, 1), 255) for t in base] for base in (QUANT_LUMA, QUANT_CHROMA)]


def huff_codes(table):
    """{symbol: (code, length)} of a (BITS, HUFFVAL) table (T.81 Annex C)."""
    bits, vals = table
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return codes


def header(h, w, quality, restart_mcus):
    """SOI, APP0 (JFIF 1.01, density 1:1), DQT 0, DQT 1, SOF0, DHT x 4, DRI, SOS header."""
    if not (1 <= h <= 65535 and 1 <= w <= 65535 and 1 <= restart_mcus <= 65535):
        raise ValueError("bad dimensions or restart interval")
    luma, chroma = scaled_tables(quality)
    out = bytearray(b"\xff\xd8")
    out += b"\xff\xe0" + struct.pack(">H5sBBBHHBB", 16, b"JFIF\0", 1, 1, 0, 1, 1, 0, 0)
    for tq, table in ((0, luma), (1, chroma)):
        out += b"\xff\xdb" + struct.pack(">HB", 67, tq) + bytes(table[n] for n in ZIGZAG)
    out += b"\xff\xc0" + struct.pack(">HBHHB", 17, 8, h, w, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc_th, (bits, vals) in HUFF_TABLES:
        out += b"\xff\xc4" + struct.pack(">HB", 3 + 16 + len(vals), tc_th) + bytes(bits) + bytes(vals)
    out += b"\xff\xdd" + struct.pack(">HH", 4, restart_mcus)
    out += b"\xff\xda" + struct.pack(">HB", 12, 3) + bytes([1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    return bytes(out)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n  # (numpy's >> on int64 is arithmetic)


def _dct_pass(d, first):
    """One pass of the Loeffler-Ligtenberg-Moschytz DCT along the last axis of int64 [..., 8]; ``first``: the row pass (results scaled up
    by 4), else the column pass (that scale removed; the result is 8 times the orthonormal DCT)."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    shift = 11 if first else 15
    if first:
        o0, o4 = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o0, o4 = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * F_0_541196100
    o2 = _descale(z1 + t13 * F_0_765366865, shift)
    o6 = _descale(z1 - t12 * F_1_847759065, shift)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F_1_175875602
    t4, t5, t6, t7 = t4 * F_0_298631336, t5 * F_2_053119869, t6 * F_3_072711026, t7 * F_1_501321110
    z1, z2, z3, z4 = -z1 * F_0_899976223, -z2 * F_2_562915447, -z3 * F_1_961570560 + z5, -z4 * F_0_390180644 + z5
    o7, o5, o3, o1 = _descale(t4 + z1 + z3, shift), _descale(t5 + z2 + z4, shift), _descale(t6 + z2 + z3, shift), _descale(t7 + z1 + z4, shift)
    return np.stack([o0, o1, o2, o3, o4, o5, o6, o7], axis=-1)


def fdct(blocks):
    """int64 [..., 8, 8] level-shifted samples -> int64 [..., 8, 8] coefficients, 8 times the orthonormal DCT."""
    rows = _dct_pass(blocks.astype(np.int64), True)
    return np.swapaxes(_dct_pass(np.swapaxes(rows, -1, -2), False), -1, -2)


def ycbcr(rgb):
    """uint8 [..., 3] -> (Y, Cb, Cr) int64, JFIF full-range BT.601 in 16-bit fixed point."""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16
    return y, cb, cr


def coefficients(rgb, quality):
    """uint8 [h, w, 3] -> int64 [MCUs, 6, 64]: the quantised coefficients in zig-zag order, MCUs in raster order, blocks Y00 Y01 Y10 Y11
    Cb Cr (what jpeg_dct_quant_kernel leaves in the workspace)."""
    rgb = np.asarray(rgb)
    h, w, _ = rgb.shape
    mh, mw = (h + 15) // 16, (w + 15) // 16
    rgb = rgb[np.minimum(np.arange(mh * 16), h - 1)][:, np.minimum(np.arange(mw * 16), w - 1)]  # replicate the last row / column
    y, cb, cr = ycbcr(rgb)
    sub = lambda c: (c.reshape(mh * 8, 2, mw * 8, 2).sum(axis=(1, 3)) + 2) >> 2  # noqa: E731
    yb = (y - 128).reshape(mh, 2, 8, mw, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(mh * mw, 4, 8, 8)
    cbb, crb = ((sub(c) - 128).reshape(mh, 8, mw, 8).transpose(0, 2, 1, 3).reshape(mh * mw, 1, 8, 8) for c in (cb, cr))
    coef = fdct(np.concatenate([yb, cbb, crb], axis=1)).reshape(mh * mw, 6, 64)
    luma, chroma = (np.array(t, np.int64) * 8 for t in scaled_tables(quality))
    div = np.stack([luma] * 4 + [chroma] * 2)[None]
    q = np.sign(coef) * ((np.abs(coef) + div // 2) // div)
    return q[:, :, ZIGZAG]


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)  # pad with 1-bits
        return self.out


def _size_bits(v):
    size = int(abs(v)).bit_length()
    return size, (v if v >= 0 else v - 1) & ((1 << size) - 1)


def entropy_data(coef, restart_mcus):
    """The scan's bytes (intervals, RSTm markers) from int64 [MCUs, 6, 64] zig-zag coefficients."""
    dc = [huff_codes(DC_LUMA), huff_codes(DC_CHROMA)]
    ac = [huff_codes(AC_LUMA), huff_codes(AC_CHROMA)]
    out = bytearray()
    n_mcu = coef.shape[0]
    coef = coef.tolist()
    for k, first in enumerate(range(0, n_mcu, restart_mcus)):
        if k:
            out += bytes([0xFF, 0xD0 + (k - 1) % 8])
        bits, pred = _Bits(), [0, 0, 0]
        for m in range(first, min(first + restart_mcus, n_mcu)):
            for blk in range(6):
                comp = max(blk - 3, 0)
                tab = min(comp, 1)
                c = coef[m][blk]
                size, extra = _size_bits(c[0] - pred[comp])
                pred[comp] = c[0]
                bits.put(*dc[tab][size])
                bits.put(extra, size)
                run = 0
                for v in c[1:]:
                    if v == 0:
                        run += 1
                        continue
                    while run > 15:
                        bits.put(*ac[tab][0xF0])
                        run -= 16
                    size, extra = _size_bits(v)
                    bits.put(*ac[tab][run << 4 | size])
                    bits.put(extra, size)
                    run = 0
                if run:
                    bits.put(*ac[tab][0x00])
        out += bits.flush()
    return bytes(out)


def encode(rgb, quality, restart_mcus):
    """uint8 [h, w, 3] -> one baseline JPEG."""
    rgb = np.asarray(rgb)
    h, w, _ = rgb.shape
    return header(h, w, quality, restart_mcus) + entropy_data(coefficients(rgb, quality), restart_mcus) + b"\xff\xd9"


def slot_header(stream, slot_bytes):
    """The 16-byte slot header of a stream: length (LE u32), status, 8 zero bytes."""
    return struct.pack("<IIQ", len(stream), int(16 + len(stream) > slot_bytes), 0)


def walk(stream):
    """Marker walker: {"segments": [(marker, payload)] up to and including SOS, "dri", "entropy": (lo, hi) span of the entropy data,
    "rst": [(offset, m)], "stuffed": number of FF 00 pairs}.  Raises ValueError on a malformed stream: an 0xFF in the entropy data that is
    neither stuffed nor a restart marker in cyclic order, or anything behind EOI."""
    stream = bytes(stream)
    if stream[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    pos, segments, dri = 2, [], None
    while True:
        if stream[pos] != 0xFF:
            raise ValueError(f"no marker at {pos}")
        marker = stream[pos + 1]
        (length,) = struct.unpack(">H", stream[pos + 2: pos + 4])
        payload = stream[pos + 4: pos + 2 + length]
        segments.append((marker, payload))
        pos += 2 + length
        if marker == 0xDD:
            (dri,) = struct.unpack(">H", payload)
        if marker == 0xDA:
            break
    lo, rst, stuffed = pos, [], 0
    while True:
        if pos >= len(stream) - 1:
            raise ValueError("no EOI")
        if stream[pos] != 0xFF:
            pos += 1
            continue
        nxt = stream[pos + 1]
        if nxt == 0x00:
            stuffed += 1
        elif 0xD0 <= nxt <= 0xD7:
            if nxt - 0xD0 != len(rst) % 8:
                raise ValueError(f"RST{nxt - 0xD0} at {pos} out of order")
            rst.append((pos, nxt - 0xD0))
        elif nxt == 0xD9:
            break
        else:
            raise ValueError(f"unstuffed 0xFF at {pos}")
        pos += 2
    if pos + 2 != len(stream):
        raise ValueError("bytes behind EOI")
    return {"segments": segments, "dri": dri, "entropy": (lo, pos), "rst": rst, "stuffed": stuffed}


def avi_frames(path):
    """RIFF walker of an AVI 1.0 file: {"frames": [payload], "avih": dict, "strh": dict, "strf": dict, "idx1": [(ckid, flags, offset, size)],
    "movi": file offset of the 'movi' fourcc, "chunks": [(file offset of the chunk header, size)], "riff_size"}."""
    data = open(path, "rb").read()
    if data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError("not a RIFF AVI file")
    (riff_size,) = struct.unpack("<I", data[4:8])
    if riff_size + 8 != len(data):
        raise ValueError(f"RIFF size {riff_size} + 8 != file size {len(data)}")
    out = {"frames": [], "chunks": [], "idx1": [], "riff_size": riff_size}

    def chunks(lo, hi):
        while lo < hi:
            fourcc, (size,) = data[lo: lo + 4], struct.unpack("<I", data[lo + 4: lo + 8])
            if lo + 8 + size > hi:
                raise ValueError(f"chunk {fourcc!r} at {lo} leaves its parent")
            yield fourcc, lo, size
            lo += 8 + size + (size & 1)

    def visit(lo, hi):
        for fourcc, at, size in chunks(lo, hi):
            body = data[at + 8: at + 8 + size]
            if fourcc == b"LIST":
                if body[:4] == b"movi":
                    out["movi"] = at + 8
                visit(at + 12, at + 8 + size)
            elif fourcc == b"avih":
                names = ("us_per_frame", "max_bytes_per_sec", "padding", "flags", "total_frames", "initial_frames", "streams", "buffer_size",
                         "width", "height")
                out["avih"] = dict(zip(names, struct.unpack("<10I", body[:40])))
            elif fourcc == b"strh":
                f = struct.unpack("<4s4sIHHIIIIIIII", body[:48])
                out["strh"] = dict(type=f[0], handler=f[1], scale=f[6], rate=f[7], start=f[8], length=f[9], buffer_size=f[10])
            elif fourcc == b"strf":
                f = struct.unpack("<IiiHH4sI", body[:24])
                out["strf"] = dict(size=f[0], width=f[1], height=f[2], planes=f[3], bit_count=f[4], compression=f[5], image_size=f[6])
            elif fourcc == b"00dc":
                out["frames"].append(body)
                out["chunks"].append((at, size))
            elif fourcc == b"idx1":
                out["idx1"] = [struct.unpack("<4sIII", body[i: i + 16]) for i in range(0, size, 16)]

    visit(12, len(data))
    return out


SIZES = [(16, 16), (8, 8), (24, 40), (56, 120), (256, 256)]  # (h, w): one MCU; replication on both axes; partial MCUs; several rows; many


def inputs(h, w):
    """The test pictures at (h, w), uint8 [h, w, 3]: a smooth synthetic frame, uniform noise, flat 0, flat 255 and a full-amplitude
    checkerboard (8 x 8 squares on the left half: the largest DC differences; single pixels on the right half: the largest AC values)."""
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([(yy + xx) // 2 % 256, 255 - yy % 256, 128 + 100 * np.sin(xx / 20.0) * np.cos(yy / 31.0)], -1).astype(np.uint8)
    noise = np.random.default_rng(1000 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    squares = np.where(xx < max(w // 2, 8), (yy // 8 + xx // 8) % 2, (yy + xx) % 2) * 255
    checker = np.repeat(squares[..., None], 3, -1).astype(np.uint8)
    return {"smooth": smooth, "noise": noise, "flat0": np.zeros((h, w, 3), np.uint8), "flat255": np.full((h, w, 3), 255, np.uint8),
            "checker": checker}
