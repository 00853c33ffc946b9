"""Motion-JPEG in a plain AVI 1.0 container: what render_video --video mjpeg writes where the reference's .mp4 files stand.

    RIFF 'AVI '
      LIST 'hdrl':  avih (AVIF_HASINDEX, one stream),  LIST 'strl':  strh ('vids' / 'MJPG', scale 1, rate fps),  strf (BITMAPINFOHEADER, 24 bit, 'MJPG')
      LIST 'movi':  one '00dc' chunk per frame -- a complete JPEG file --, padded to even length
      idx1:         per frame '00dc', AVIIF_KEYFRAME, the chunk's offset from the 'movi' fourcc, its size

Frames are appended as they arrive; close() appends them again in reverse order (the reference's imgs += imgs[::-1]) by reading them back from the file it is
writing, so memory holds one frame and the index, never the video.  Every size field is 32 bits and players read them as signed: a file that would pass
2^31 - 1 bytes is refused (the OpenDML extension for larger files is not built).
"""
import os
import struct

LIMIT = 2 ** 31 - 1
_HEADER = 224                     # bytes in front of the first chunk; the 'movi' fourcc stands at _HEADER - 4
AVIF_HASINDEX, AVIIF_KEYFRAME = 0x10, 0x10


class AviWriter:
    def __init__(self, path, width, height, fps):
        from .. import _lib as L
        if not (0 < width <= 65535 and 0 < height <= 65535 and fps > 0 and int(fps) == fps):
            raise L.IrisError(f"AviWriter: {width} x {height} at {fps} fps: sides of 1..65535 and a positive whole frame rate")
        self.path, self.width, self.height, self.fps = path, int(width), int(height), int(fps)
        self.sizes, self.movi_bytes = [], 0       # per chunk its data size; bytes of all chunks with their headers and padding
        self.fh = open(path + ".part", "w+b")
        self.fh.write(self._header())

    def _file_bytes(self, movi_bytes, n_chunks):
        return _HEADER + movi_bytes + 8 + 16 * n_chunks

    def _reserve(self, length):
        """account for one more chunk of `length` data bytes; refuses the chunk that would take the finished file past 2^31 - 1 bytes"""
        from .. import _lib as L
        chunk = 8 + length + length % 2
        if self._file_bytes(self.movi_bytes + chunk, len(self.sizes) + 1) > LIMIT:
            raise L.IrisError(f"AviWriter: {self.path} would pass 2^31 - 1 bytes with frame {len(self.sizes)}: an AVI 1.0 file cannot (OpenDML, for larger files, is not built); "
                              "render fewer frames, a smaller image or a lower --video_quality")
        self.sizes.append(length)
        self.movi_bytes += chunk

    def _header(self):
        n = len(self.sizes)
        biggest = max(self.sizes, default=0)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG", self.width * self.height * 3, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIiI4H", b"vids", b"MJPG", 0, 0, 0, 0, 1, self.fps, 0, n, biggest, -1, 0, 0, 0, self.width, self.height)
        avih = struct.pack("<14I", 1000000 // self.fps, 0, 0, AVIF_HASINDEX, n, 0, 1, biggest, self.width, self.height, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        head = b"RIFF" + struct.pack("<I", self._file_bytes(self.movi_bytes, n) - 8) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl
        head += b"LIST" + struct.pack("<I", 4 + self.movi_bytes) + b"movi"
        assert len(head) == _HEADER
        return head

    def add_frame(self, jpeg_bytes):
        data = bytes(jpeg_bytes)
        self._reserve(len(data))
        self.fh.write(b"00dc" + struct.pack("<I", len(data)) + data + b"\0" * (len(data) % 2))

    def close(self, reverse=True):
        """reverse: the frames once more, last to first (2 N frames); then idx1, the sizes and counts of the headers, and the file under its name"""
        try:
            forward = list(self.sizes)
            if reverse:
                from .. import _lib as L
                if self._file_bytes(2 * self.movi_bytes, 2 * len(forward)) > LIMIT:
                    raise L.IrisError(f"AviWriter: {self.path} with its frames repeated in reverse would pass 2^31 - 1 bytes: an AVI 1.0 file cannot (OpenDML, for larger "
                                      "files, is not built); render fewer frames, a smaller image or a lower --video_quality")
                starts, o = [], _HEADER
                for s in forward:
                    starts.append(o)
                    o += 8 + s + s % 2
                for start, s in zip(reversed(starts), reversed(forward)):
                    self.fh.seek(start)
                    chunk = self.fh.read(8 + s + s % 2)
                    self.fh.seek(0, os.SEEK_END)
                    self._reserve(s)
                    self.fh.write(chunk)
            self.fh.seek(0, os.SEEK_END)
            index, o = [], 4
            for s in self.sizes:
                index.append(struct.pack("<4sIII", b"00dc", AVIIF_KEYFRAME, o, s))
                o += 8 + s + s % 2
            self.fh.write(b"idx1" + struct.pack("<I", 16 * len(index)) + b"".join(index))
            self.fh.seek(0)
            self.fh.write(self._header())
            self.fh.close()
        except BaseException:
            self.fh.close()
            os.remove(self.path + ".part")
            raise
        os.replace(self.path + ".part", self.path)
