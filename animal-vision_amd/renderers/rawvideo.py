"""Raw (headerless) video reader and writer: frames back to back in one of yuv.PIX_FMTS, nothing else in the file.

It is what `ffmpeg -f rawvideo -pix_fmt nv12` writes and what a hardware decoder dumps; the format and the frame size are not in
the stream, so they are named by arguments.

  * A regular file is index-addressed by arithmetic: frame k sits at k * frame_size, so rank r of `world` reads frames
    i = r (mod world) only.  A file whose size is not a whole number of frames raises.
  * `-` (stdin / stdout) and FIFOs are read and written in order, one rank only; a stream that ends inside a frame raises,
    naming the frame."""
from __future__ import annotations

import os
import sys
from typing import BinaryIO, Optional

import numpy as np

from ..yuv import frame_size
from .y4m import _is_stream


class RawVideoReader:
    """Frames of one raw video file or stream as flat uint8 payloads (frame_size bytes each).

    rank / world: serve only frames i with i % world == rank (regular files only)."""

    def __init__(self, path: str, pix_fmt: str, width: int, height: int, *, rank: int = 0, world: int = 1):
        if not (0 <= rank < world):
            raise ValueError(f"rank {rank} outside world {world}")
        if width < 1 or height < 1:
            raise ValueError(f"raw video needs a positive size (got {width}x{height})")
        self.path, self.pix_fmt, self.width, self.height = path, pix_fmt, int(width), int(height)
        self.rank, self.world = int(rank), int(world)
        self.frame_size = frame_size(pix_fmt, self.height, self.width)
        self.sequential = _is_stream(path)
        if self.sequential and world > 1:
            raise ValueError(f"{path!r} is a pipe: it can only be read in order by one rank (world = 1), not world = {world}")
        self._f: Optional[BinaryIO] = sys.stdin.buffer if path == "-" else open(path, "rb")
        self.total_frames: Optional[int] = None
        if not self.sequential:
            size = os.fstat(self._f.fileno()).st_size
            if size % self.frame_size:
                self._f.close()
                raise ValueError(f"{path}: {size} bytes is not a whole number of {self.width}x{self.height} {pix_fmt} frames "
                                 f"({self.frame_size} bytes each)")
            self.total_frames = size // self.frame_size
        self._next = self.rank  # global index of the next frame this reader serves
        self.last_index = -1

    def read(self) -> Optional[np.ndarray]:
        """The next frame this rank serves as a flat uint8 payload (last_index = its global index), or None at the end."""
        fsz = self.frame_size
        if self.total_frames is not None:
            if self._next >= self.total_frames:
                return None
            self._f.seek(self._next * fsz)
        buf = np.empty(fsz, np.uint8)
        mv, got = memoryview(buf), 0
        while got < fsz:  # a pipe may return a frame in pieces
            n = self._f.readinto(mv[got:])
            if not n:
                break
            got += n
        if got == 0 and self.total_frames is None:
            return None
        if got != fsz:
            raise ValueError(f"{self.path}: frame {self._next} is truncated ({got} of {fsz} bytes)")
        self.last_index = self._next
        self._next += self.world
        return buf

    def close(self) -> None:
        if self._f is not None and self.path != "-":
            self._f.close()
        self._f = None


class RawVideoWriter:
    """Writes one payload per write(), nothing between them."""

    def __init__(self, path: str, pix_fmt: str, width: int, height: int):
        self.path, self.pix_fmt, self.width, self.height = path, pix_fmt, int(width), int(height)
        self.frame_size = frame_size(pix_fmt, self.height, self.width)
        self._f: Optional[BinaryIO] = sys.stdout.buffer if path == "-" else open(path, "wb")
        self.frames = 0

    def write(self, payload: np.ndarray) -> None:
        a = np.ascontiguousarray(payload, dtype=np.uint8).reshape(-1)
        if a.size != self.frame_size:
            raise ValueError(f"frame of {a.size} bytes; the {self.width}x{self.height} {self.pix_fmt} stream takes {self.frame_size}")
        self._f.write(memoryview(a))
        self.frames += 1

    def flush(self) -> None:
        if self._f is not None:
            self._f.flush()

    def close(self) -> None:
        if self._f is None:
            return
        self._f.flush()
        if self.path != "-":
            self._f.close()
        self._f = None
