"""YUV4MPEG2 (.y4m) reader and writer: a text header, then raw 8-bit planar 4:2:0 frames, each behind a `FRAME` line.

Every ffmpeg build reads and writes it, pipes included (`ffmpeg -i in.mp4 -f yuv4mpegpipe -`), so it is how real footage gets
in and out without a codec here.

  * Header `YUV4MPEG2 W<w> H<h> F<n>:<d> I<i> A<n>:<d> C<c> X<x>...`: every token is kept, unknown ones included, and written
    back in order.  `XCOLORRANGE=FULL|LIMITED` names the range (limited when absent).  Only 8-bit 4:2:0 (`C420jpeg`,
    `C420mpeg2`, `C420paldv`, `C420`, or no C tag) and progressive or unknown interlacing (`Ip`, `I?`, or no I tag) are
    accepted; any other C or I value raises ValueError naming it.  Chroma siting is accepted and ignored.
  * A regular file is index-addressed: the frame offsets are found once (by arithmetic when the first frame header is a bare
    `FRAME`; by one scan of the headers when frames carry parameters), so rank r of `world` reads frames i = r (mod world) only.
  * `-` (stdin / stdout) and FIFOs are read and written in order, one rank only.
  * The writer emits bare `FRAME` lines, so every frame of its output has the same size."""
from __future__ import annotations

import os
import stat
import sys
from dataclasses import dataclass, field
from typing import BinaryIO, List, Optional

import numpy as np

from ..yuv import i420_size

MAGIC = b"YUV4MPEG2"
FRAME = b"FRAME"
_OK_C = ("420jpeg", "420mpeg2", "420paldv", "420")
_OK_I = ("p", "?")
_MAX_LINE = 1 << 16


@dataclass
class Y4MHeader:
    """The stream header: size, and every token as it was read (tokens[k] = tag letter + value, W and H included)."""

    width: int
    height: int
    tokens: List[str] = field(default_factory=list)

    @property
    def full_range(self) -> bool:
        return self.tag("XCOLORRANGE=") == "FULL"

    @property
    def frame_size(self) -> int:
        return i420_size(self.height, self.width)

    def tag(self, prefix: str) -> Optional[str]:
        """The value after `prefix` of the first token that starts with it (e.g. tag("F") -> "30000:1001"), else None."""
        for t in self.tokens:
            if t.startswith(prefix):
                return t[len(prefix):]
        return None

    def replaced(self, prefix: str, value: Optional[str]) -> "Y4MHeader":
        """A copy with the token starting with `prefix` set to prefix + value (appended when missing; removed when value is None)."""
        toks, done = [], False
        for t in self.tokens:
            if t.startswith(prefix):
                if value is not None and not done:
                    toks.append(prefix + value)
                done = True
            else:
                toks.append(t)
        if not done and value is not None:
            toks.append(prefix + value)
        w = int(value) if prefix == "W" and value is not None else self.width
        h = int(value) if prefix == "H" and value is not None else self.height
        return Y4MHeader(w, h, toks)

    def with_size(self, width: int, height: int) -> "Y4MHeader":
        return self.replaced("W", str(int(width))).replaced("H", str(int(height)))

    def encode(self) -> bytes:
        return b" ".join([MAGIC] + [t.encode("ascii") for t in self.tokens]) + b"\n"


def parse_header(line: bytes) -> Y4MHeader:
    """One header line (with or without its newline) -> Y4MHeader; ValueError for what this reader does not take."""
    line = line.rstrip(b"\n")
    parts = line.split(b" ")
    if parts[0] != MAGIC:
        raise ValueError("not a YUV4MPEG2 stream (the header must start with 'YUV4MPEG2 ')")
    toks = [p.decode("ascii") for p in parts[1:] if p]
    w = h = None
    for t in toks:
        if t[0] == "W":
            w = int(t[1:])
        elif t[0] == "H":
            h = int(t[1:])
        elif t[0] == "C" and t[1:] not in _OK_C:
            raise ValueError(f"Y4M colour space tag {t!r} is not supported: 8-bit 4:2:0 only ({', '.join('C' + c for c in _OK_C)})")
        elif t[0] == "I" and t[1:] not in _OK_I:
            raise ValueError(f"Y4M interlacing tag {t!r} is not supported: progressive only (Ip, I?)")
        elif t.startswith("XCOLORRANGE=") and t[12:] not in ("FULL", "LIMITED"):
            raise ValueError(f"Y4M tag {t!r}: XCOLORRANGE is FULL or LIMITED")
    if not w or not h or w < 1 or h < 1:
        raise ValueError("Y4M header lacks a positive W and H")
    return Y4MHeader(w, h, toks)


def default_header(width: int, height: int, *, fps: int = 30, full_range: bool = False) -> Y4MHeader:
    """The header written when the source has none: progressive, square pixels, C420jpeg."""
    toks = [f"W{width}", f"H{height}", f"F{int(fps)}:1", "Ip", "A1:1", "C420jpeg"]
    if full_range:
        toks.append("XCOLORRANGE=FULL")
    return Y4MHeader(width, height, toks)


def _is_stream(path: str) -> bool:
    return path == "-" or (os.path.exists(path) and stat.S_ISFIFO(os.stat(path).st_mode))


def _readline(f: BinaryIO) -> bytes:
    line = f.readline(_MAX_LINE)
    if line and not line.endswith(b"\n"):
        raise ValueError("Y4M header line is not terminated (or is longer than 64 KiB)")
    return line


def _frame_line(line: bytes, where: str) -> None:
    if not (line == FRAME + b"\n" or line.startswith(FRAME + b" ")):
        raise ValueError(f"Y4M {where}: expected a FRAME header, got {line[:32]!r}")


class Y4MReader:
    """Frames of one .y4m file or stream as flat uint8 I420 payloads (header.frame_size bytes each).

    rank / world: serve only frames i with i % world == rank (regular files only)."""

    def __init__(self, path: str, *, rank: int = 0, world: int = 1):
        if not (0 <= rank < world):
            raise ValueError(f"rank {rank} outside world {world}")
        self.path, self.rank, self.world = path, int(rank), int(world)
        self.sequential = _is_stream(path)
        if self.sequential and world > 1:
            raise ValueError(f"{path!r} is a pipe: it can only be read in order by one rank (world = 1), not world = {world}")
        self._f: BinaryIO = sys.stdin.buffer if path == "-" else open(path, "rb")
        self.header = parse_header(_readline(self._f))
        self.offsets: Optional[List[int]] = None  # payload offset of every frame (regular files)
        self._next = self.rank                    # global index of the next frame this reader serves
        self._bare = False                        # frame offsets by arithmetic (frame 0 has a bare FRAME header)
        self.last_index = -1
        if not self.sequential:
            self._index()

    @property
    def total_frames(self) -> Optional[int]:
        return None if self.offsets is None else len(self.offsets)

    def _index(self) -> None:
        f, fsz = self._f, self.header.frame_size
        data0 = f.tell()
        end = os.fstat(f.fileno()).st_size
        first = _readline(f)
        offsets: List[int] = []
        if not first:
            self.offsets = offsets
            return
        _frame_line(first, "frame 0")
        step = len(first) + fsz
        if first == FRAME + b"\n" and (end - data0) % step == 0:
            # bare headers: frame k sits at data0 + k * step; each one's header is checked when it is read
            offsets = [data0 + k * step + len(first) for k in range((end - data0) // step)]
            self._bare = True
        else:  # frame parameters: one scan of the frame headers
            pos, line = data0, first
            while line:
                _frame_line(line, f"frame {len(offsets)}")
                pos += len(line)
                if pos + fsz > end:
                    raise ValueError(f"{self.path}: frame {len(offsets)} is truncated")
                offsets.append(pos)
                pos += fsz
                f.seek(pos)
                line = _readline(f)
        self.offsets = offsets

    def read(self) -> Optional[np.ndarray]:
        """The next frame this rank serves as a flat uint8 payload (last_index = its global index), or None at the end."""
        fsz = self.header.frame_size
        if self.offsets is not None:
            if self._next >= len(self.offsets):
                return None
            off = self.offsets[self._next]
            if self._bare:  # offsets by arithmetic: this frame's header must be a bare FRAME too
                self._f.seek(off - len(FRAME) - 1)
                if self._f.read(len(FRAME) + 1) != FRAME + b"\n":
                    raise ValueError(f"{self.path}: frame {self._next} does not have a bare FRAME header where frame 0 did")
            self._f.seek(off)
        else:
            line = _readline(self._f)
            if not line:
                return None
            _frame_line(line, f"frame {self._next}")
        buf = np.empty(fsz, np.uint8)
        got = self._f.readinto(memoryview(buf)) if self.offsets is not None else self._read_all(buf)
        if got != fsz:
            raise ValueError(f"{self.path}: frame {self._next} is truncated ({got} of {fsz} bytes)")
        self.last_index = self._next
        self._next += self.world
        return buf

    def _read_all(self, buf: np.ndarray) -> int:
        """A pipe may return a frame in pieces."""
        mv, got = memoryview(buf), 0
        while got < len(buf):
            n = self._f.readinto(mv[got:])
            if not n:
                break
            got += n
        return got

    def close(self) -> None:
        if self._f is not None and self.path != "-":
            self._f.close()
        self._f = None


class Y4MWriter:
    """Writes `header` and then one bare `FRAME` + payload per write()."""

    def __init__(self, path: str, header: Y4MHeader):
        self.path, self.header = path, header
        self._f: Optional[BinaryIO] = sys.stdout.buffer if path == "-" else open(path, "wb")
        self._f.write(header.encode())
        self.frames = 0

    def write(self, payload: np.ndarray) -> None:
        a = np.ascontiguousarray(payload, dtype=np.uint8).reshape(-1)
        if a.size != self.header.frame_size:
            raise ValueError(f"frame of {a.size} bytes; the {self.header.width}x{self.header.height} stream takes {self.header.frame_size}")
        self._f.write(FRAME + b"\n")
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
