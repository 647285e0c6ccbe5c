"""Motion-JPEG in an AVI 1.0 container, written by the host alone (no encoder, no torch): what FrameSink(pix_fmt="mjpeg") falls back to
when there is no ``ffmpeg`` binary.  Every frame is one complete baseline JPEG (csrc/jpeg.hip) and goes into the file as it is.

    RIFF 'AVI '
      LIST 'hdrl'   avih | LIST 'strl' ( strh vids / MJPG | strf BITMAPINFOHEADER )
      LIST 'movi'   00dc chunks, padded to even sizes
      idx1          one entry per chunk: offset from the 'movi' fourcc, size

The frame rate is dwRate / dwScale with dwScale = 1000000.  Sizes and frame counts are patched on close().  RIFF sizes are 32 bits wide:
when the next chunk and its index entry would take the file past RIFF_LIMIT, the writer finishes the file and continues in
``<stem>.002.avi``, ``<stem>.003.avi``, ... (no OpenDML index).  Audio is not muxed.
"""
import struct

RIFF_LIMIT = 0xFFF00000
SCALE = 1000000
_AVIF_HASINDEX, _AVIIF_KEYFRAME = 0x10, 0x10
_HEADER_BYTES = 12 + 12 + (8 + 56) + 12 + (8 + 56) + (8 + 40) + 12  # RIFF, hdrl, avih, strl, strh, strf, LIST movi


class MjpegAviWriter:
    """``write(payload)`` appends one JPEG; ``close()`` finishes the (last) file.  ``paths``: the files written so far, ``count``: frames."""

    def __init__(self, path, width, height, framerate):
        rate = int(round(float(framerate) * SCALE))
        if not (0 < rate < 1 << 32) or not (0 < width < 1 << 16 and 0 < height < 1 << 16):
            raise ValueError(f"cannot describe {width}x{height} at {framerate} frames/s in an AVI header")
        self.w, self.h, self.rate, self.framerate = int(width), int(height), rate, float(framerate)
        self.stem = path[:-4] if path.lower().endswith(".avi") else path
        self.paths, self.count = [], 0
        self.file = None
        self._open()

    def _open(self):
        part = len(self.paths) + 1
        path = f"{self.stem}.avi" if part == 1 else f"{self.stem}.{part:03d}.avi"
        self.paths.append(path)
        self.file = open(path, "wb")
        self.index, self.largest = [], 0
        self.file.write(self._headers(0, 0))
        self.pos = _HEADER_BYTES

    def _headers(self, frames, movi_bytes):
        """Everything in front of the first chunk; ``movi_bytes``: size of the LIST 'movi' (its fourcc + the chunks)."""
        us_per_frame = int(round(1e6 / self.framerate))
        bytes_per_sec = int(self.largest * self.framerate) & 0xFFFFFFFF
        avih = struct.pack("<14I", us_per_frame, bytes_per_sec, 0, _AVIF_HASINDEX, frames, 0, 1, self.largest, self.w, self.h, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIIIhhhh", b"vids", b"MJPG", 0, 0, 0, 0, SCALE, self.rate, 0, frames, self.largest, 0xFFFFFFFF, 0,
                           0, 0, self.w, self.h)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.w, self.h, 1, 24, b"MJPG", self.w * self.h * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        riff_size = _HEADER_BYTES - 8 + (movi_bytes - 4) + 8 + 16 * frames
        head = (b"RIFF" + struct.pack("<I", riff_size) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl
                + b"LIST" + struct.pack("<I", movi_bytes) + b"movi")
        assert len(head) == _HEADER_BYTES
        return head

    def write(self, payload):
        payload = memoryview(payload).cast("B")
        size = len(payload)
        padded = size + (size & 1)
        if self.index and self.pos + 8 + padded + 8 + 16 * (len(self.index) + 1) > RIFF_LIMIT:
            self._finish()
            self._open()
        self.file.write(b"00dc" + struct.pack("<I", size))
        self.file.write(payload)
        if size & 1:
            self.file.write(b"\0")
        self.index.append((self.pos - (_HEADER_BYTES - 4), size))  # offsets count from the 'movi' fourcc
        self.largest = max(self.largest, size)
        self.pos += 8 + padded
        self.count += 1

    def _finish(self):
        idx = b"".join(struct.pack("<4sIII", b"00dc", _AVIIF_KEYFRAME, offset, size) for offset, size in self.index)
        self.file.write(b"idx1" + struct.pack("<I", len(idx)) + idx)
        self.file.seek(0)
        self.file.write(self._headers(len(self.index), 4 + self.pos - _HEADER_BYTES))
        self.file.close()
        self.file = None

    def close(self):
        if self.file is not None:
            self._finish()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
