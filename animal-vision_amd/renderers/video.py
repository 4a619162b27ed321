"""VideoRenderer -- the frame source/sink of the reference's renderers/video.py with its keyword surface
(`read_path, write_path, fps, window_name`, :31-38) and frame contract (RGB uint8 HxWx3 from get_image(),
None at end of stream, :82-96).

Codec I/O is out of scope (the reference leans on cv2.VideoCapture / VideoWriter 'mp4v', :68,:113; neither
cv2 nor ffmpeg exists here), so paths name what this box can read and write:
  read_path : "synthetic:<W>x<H>:<n>[:noise|structured]"  |  a .npy file (N,H,W,3 uint8)  |  a directory of images
              |  a .y4m file or "-" (stdin / a FIFO: YUV4MPEG2, 8-bit 4:2:0, what `ffmpeg -f yuv4mpegpipe` writes)
  write_path: a directory (one PNG per frame, via Pillow)  |  a .npy file  |  a .y4m file or "-" (stdout)  |  None
No preview window (no GUI); `window_name` is accepted and ignored.

Y4M (renderers/y4m.py): get_image() still returns RGB uint8 HxWx3, converted from the I420 payload on the device (yuv.py);
get_yuv() hands over the payload itself, and render() takes RGB frames (converted on the device) or payloads.  `matrix` and
`range` name the conversion; range None = the source's XCOLORRANGE tag, else limited.  Every conversion goes through
the `decode` and `encode` properties (yuv.Decode, yuv.Encode), which the constructor's settings are made into once.  The sink
echoes the source's header (size, rate, aspect, colour range, unknown tags) when the source is a .y4m.

Raw video (renderers/rawvideo.py): `pix_fmt` and `size=(W, H)` read `read_path` (a file, "-" or a FIFO) as headerless
frames in one of yuv.PIX_FMTS (nv12, p010le, yuv422p, ...); `write_pix_fmt` writes `write_path` the same way, and defaults to
`pix_fmt` when the sink is "-" or ends in .yuv.  get_image() and get_yuv() keep their contracts; a raw source into a .y4m sink
goes through RGB.

HDR sources: `transfer` ("pq" or "hlg") reads a raw 10-bit source as BT.2020 HDR video.  get_image() then returns
the tone-mapped SDR frame of the HDR decode (`tonemap`, `peak_nits`, `sdr_white`; `matrix` plays no part in the decode), so
the per-frame species get it too, and every YUV sink is encoded in `out_matrix`: "bt709" by default with a transfer, `matrix`
without one.

Scaling: `scale=(Wd, Hd)` reduces every source's frames to Wd x Hd (cv2's INTER_AREA; enlarging is refused).
get_image() returns scaled frames -- raw and .y4m sources, HDR ones too, through the scaled decode, which goes
straight to the scaled frame; the other sources through the resize alone.  get_yuv() still hands over source-size payloads and
`yuv_hw` still names the source size (pipeline.run_video reduces them as it decodes); `out_hw` names the size of what comes out,
and every sink is written at that size -- unless the operator that runs between source and sink has an output size of its own (the
species wall): set_output_size() then names the sinks' size (`sink_hw`).

Sharded streams (two keywords the reference does not have, both defaulted): with `world` > 1 this renderer
serves and stores only the frames of rank `rank` (global frame i belongs to rank i mod world) -- every source here is
index-addressable, so the other ranks' frames are never generated, read or decoded.  Outputs carry the GLOBAL frame
index: PNG sinks are named frame_<global index>.png (ranks may share the directory); a .npy sink is written as one
memory-mapped shard per rank (streamed to disk frame by frame, never held in RAM) and rank 0's merge_shards() -- called
by pipeline.run_video after the ranks' closing collective -- interleaves them into the one ordered stream."""
from __future__ import annotations

import dataclasses
import os
from typing import List, Optional

import numpy as np

from ..synthetic import SyntheticVideoSource
from .renderer import Renderer


def _resize_area_u8(img: np.ndarray, W: int, H: int) -> np.ndarray:
    """cv2.resize(img, (W, H), interpolation=cv2.INTER_AREA) of a uint8 frame on the device (csrc/geom.hip)."""
    from ..geometry import INTER_AREA, resize

    return resize(np.ascontiguousarray(img), (W, H), INTER_AREA)


def split_compose(original: np.ndarray, modified: np.ndarray, draw_seam: bool = True, *, left_label: Optional[str] = None,
                  right_label: Optional[str] = None) -> np.ndarray:
    """renderers/video.py:225-245: `modified` resized to `original`'s size if needed (INTER_AREA, on the device), left half
    original, right half modified, 1-px white seam at W//2, then the two corner labels (None = no label)."""
    assert isinstance(original, np.ndarray) and original.ndim == 3 and original.shape[2] == 3, "original must be HxWx3 RGB"
    assert isinstance(modified, np.ndarray) and modified.ndim == 3 and modified.shape[2] == 3, "modified must be HxWx3 RGB"
    H, W, _ = original.shape
    if modified.shape[:2] != (H, W):
        if original.dtype != np.uint8 or modified.dtype != np.uint8:
            raise TypeError("split compare of frames of different sizes is implemented for uint8 frames (what get_image() yields)")
        modified = _resize_area_u8(modified, W, H)
    out = original.copy()
    mid = W // 2
    out[:, mid:, :] = modified[:, mid:, :]
    if draw_seam:
        out[:, mid : mid + 1, :] = 255
    if left_label is not None or right_label is not None:
        from .labels import draw_split_labels

        out = draw_split_labels(out, left_label, right_label)
    return out


def is_raw_sink(path: Optional[str]) -> bool:
    """A path that is written as raw video when the source's pix_fmt is known and no write_pix_fmt is given: "-" or *.yuv."""
    return bool(path) and (path == "-" or path.lower().endswith(".yuv"))


def is_y4m(path: Optional[str]) -> bool:
    """A path the Y4M reader / writer serves: "-" (stdin / stdout) or a name ending in .y4m."""
    return bool(path) and (path == "-" or path.lower().endswith(".y4m"))


class VideoRenderer(Renderer):
    def __init__(self, *, read_path: Optional[str] = None, write_path: Optional[str] = None, fps: Optional[int] = None,
                 window_name: str = "Video Analysis", rank: int = 0, world: int = 1, matrix: str = "bt601", range: Optional[str] = None,
                 pix_fmt: Optional[str] = None, size: Optional[tuple] = None, write_pix_fmt: Optional[str] = None,
                 transfer: Optional[str] = None, tonemap: str = "mobius", peak_nits: float = 1000.0, sdr_white: float = 203.0,
                 out_matrix: Optional[str] = None, scale: Optional[tuple] = None):
        if not (0 <= rank < world):
            raise ValueError(f"rank {rank} outside world {world}")
        if (pix_fmt is None) != (size is None):
            raise ValueError("a raw video source is named by both pix_fmt and size=(W, H)")
        if write_pix_fmt is None and pix_fmt is not None and is_raw_sink(write_path):
            write_pix_fmt = pix_fmt
        from ..yuv import codec

        # the settings of every conversion, checked here; the range may still come from a .y4m header (the decode and encode properties)
        self._decode, enc = codec(pix_fmt, matrix, range or "limited", transfer, tonemap, peak_nits, sdr_white, out_matrix, scale)
        self._encode = dataclasses.replace(enc, pix_fmt=write_pix_fmt if write_path else pix_fmt)  # the sink's format; the source's without a sink
        if write_pix_fmt is not None and not write_path:
            raise ValueError("write_pix_fmt needs a write_path")
        self.transfer, self.tonemap, self.peak_nits, self.sdr_white, self.out_matrix = transfer, tonemap, float(peak_nits), float(sdr_white), enc.matrix
        self.pix_fmt, self.write_pix_fmt = pix_fmt, write_pix_fmt
        self.size = None if size is None else (int(size[0]), int(size[1]))
        if scale is not None:
            # a raw source names its size here; the other sources are checked when their size is known (open(), get_image())
            Ws, Hs = self.size or self._decode.scale
            Hd, Wd = self._decode.out_hw(Hs, Ws)
            scale = (Wd, Hd)
        self.scale = scale
        self._raw = None             # renderers.rawvideo.RawVideoReader
        self._raw_out = None         # renderers.rawvideo.RawVideoWriter (created by the first render)
        self._merge_size = self.scale or self.size  # (W, H) of the raw sink's frames, for merge_shards()
        self._sink_hw = None         # set_output_size(): the sinks' frame size where it is not out_hw
        if write_path == "-" and world > 1:
            raise ValueError("stdout is one ordered stream: it can only be written with world = 1")
        self.read_path, self.write_path = read_path, write_path
        self.fps = fps or 30
        self.window_name = window_name
        self.rank, self.world = int(rank), int(world)
        self._src = None
        self._frames: Optional[np.ndarray] = None
        self._files: List[str] = []
        self._i = self.rank          # global index of the next frame this rank reads
        self.last_index = -1         # global index of the frame get_image() returned last
        self.total_frames: Optional[int] = None
        self._sink = None            # memory-mapped .npy shard (streamed)
        self._sink_rows = 0
        self.frames_written = 0
        self.matrix, self._range = matrix, range
        self._y4m = None             # renderers.y4m.Y4MReader
        self._y4m_out = None         # renderers.y4m.Y4MWriter (created by the first render)

    # ---- source ----------------------------------------------------------------------------------------
    def open(self) -> None:
        p = self.read_path
        if p:
            if self.pix_fmt is not None:
                from .rawvideo import RawVideoReader

                self._raw = RawVideoReader(p, self.pix_fmt, self.size[0], self.size[1], rank=self.rank, world=self.world)
                self.total_frames = self._raw.total_frames
            elif is_y4m(p):
                from .y4m import Y4MReader

                self._y4m = Y4MReader(p, rank=self.rank, world=self.world)
                self.total_frames = self._y4m.total_frames
                self._check_scale(self._y4m.header.height, self._y4m.header.width)
            elif p.startswith("synthetic:"):
                parts = p.split(":")
                w, h = (int(v) for v in parts[1].lower().split("x"))
                kind = parts[3] if len(parts) > 3 else "noise"
                self.total_frames = int(parts[2])
                self._src = SyntheticVideoSource(h, w, self.total_frames, kind, offset=self.rank, stride=self.world)
            elif p.endswith(".npy"):
                self._frames = np.load(p, mmap_mode="r")
                self.total_frames = len(self._frames)
            elif os.path.isdir(p):
                self._files = sorted(os.path.join(p, f) for f in os.listdir(p) if f.lower().endswith((".png", ".jpg", ".jpeg")))
                self.total_frames = len(self._files)
            else:
                raise RuntimeError(f"Failed to open video for reading: {p} (no codec on this box: synthetic:, .npy or an image directory)")
        if self.write_path and not self.write_path.endswith(".npy") and not is_y4m(self.write_path) and self.write_pix_fmt is None:
            os.makedirs(self.write_path, exist_ok=True)

    @property
    def yuv_range(self) -> str:
        """The YUV range of the conversions: the constructor's, else the .y4m source's XCOLORRANGE tag, else limited."""
        if self._range is not None:
            return self._range
        return "full" if self._y4m is not None and self._y4m.header.full_range else "limited"

    @property
    def decode(self):
        """The yuv.Decode of this source's payloads (raw video, or the I420 of a .y4m) into the frames get_image() returns: what
        get_image() runs, and what pipeline.run_video and the pair commands launch on payloads they upload themselves.  Read it after
        open(): the range may be the .y4m header's."""
        return dataclasses.replace(self._decode, range=self.yuv_range)

    @property
    def encode(self):
        """The yuv.Encode of RGB frames into what the sink takes -- write_pix_fmt, else I420 -- or, without a sink, into the source's
        format (payloads in, payloads out), in `out_matrix`.  Read it after open(), as `decode`."""
        return dataclasses.replace(self._encode, range=self.yuv_range)

    @property
    def y4m_header(self):
        """The .y4m source's header (renderers.y4m.Y4MHeader), None for other sources."""
        return None if self._y4m is None else self._y4m.header

    @property
    def yuv_hw(self) -> Optional[tuple]:
        """(H, W) when frames can stay I420 end to end -- a .y4m source and a .y4m sink (or none) -- else None.
        pipeline.run_video then streams get_yuv() payloads (FramePipeline io_format="i420")."""
        if self._raw is not None:
            if self.write_path and self.write_pix_fmt != self.pix_fmt:
                return None
            return self._raw.height, self._raw.width
        if self._y4m is None or self.write_pix_fmt is not None or (self.write_path and not is_y4m(self.write_path)):
            return None
        return self._y4m.header.height, self._y4m.header.width

    def _check_scale(self, H: int, W: int) -> None:
        if self.scale is not None:
            from ..yuv import check_scale

            check_scale(H, W, self.scale[1], self.scale[0])

    @property
    def out_hw(self) -> Optional[tuple]:
        """(H, W) of the frames get_image() returns and of everything the sinks are handed: `scale` when it is set, else the
        source's size when it is known before the first frame (raw and .y4m sources), else None."""
        if self.scale is not None:
            return self.scale[1], self.scale[0]
        if self._raw is not None:
            return self._raw.height, self._raw.width
        if self._y4m is not None:
            return self._y4m.header.height, self._y4m.header.width
        return None

    def set_output_size(self, H: int, W: int) -> None:
        """The size of what the sinks are handed when it is not the size of the frames read: an operator with a size of its own
        (pipeline.FramePipeline with an op that has out_shape, e.g. the species wall).  pipeline.run_video calls it with the
        pipeline's out_H, out_W; payloads rendered afterwards, and the header of a sink that no frame reached, have this size."""
        self._sink_hw = (int(H), int(W))
        self._merge_size = (int(W), int(H))

    @property
    def sink_hw(self) -> Optional[tuple]:
        """(H, W) of what the sinks are handed: set_output_size()'s, else out_hw."""
        return self._sink_hw if self._sink_hw is not None else self.out_hw

    def _scaled(self, f: Optional[np.ndarray]) -> Optional[np.ndarray]:
        """An RGB frame of the source's size reduced to `scale` (INTER_AREA on the device)."""
        if f is None or self.scale is None:
            return f
        self._check_scale(f.shape[0], f.shape[1])
        if f.shape[:2] == (self.scale[1], self.scale[0]):
            return f
        return _resize_area_u8(f, self.scale[0], self.scale[1])

    @property
    def yuv_pix_fmt(self) -> Optional[str]:
        """The raw pixel format of the payloads get_yuv() hands over when `yuv_hw` is set; None = I420 (.y4m)."""
        return self.pix_fmt if self._raw is not None else None

    def get_yuv(self) -> Optional[np.ndarray]:
        """The next frame of a .y4m or raw source as its flat uint8 payload, None at end of stream."""
        if self._raw is not None:
            f = self._raw.read()
            if f is not None:
                self.last_index = self._raw.last_index
            return f
        if self._y4m is None:
            raise RuntimeError("get_yuv() needs a .y4m (or '-') or raw video source")
        f = self._y4m.read()
        if f is not None:
            self.last_index = self._y4m.last_index
        return f

    def get_image(self) -> Optional[np.ndarray]:
        if self._raw is not None or self._y4m is not None:
            f = self.get_yuv()
            if f is None:
                return None
            src = self._raw if self._raw is not None else self._y4m.header
            return self.decode.arrays(f, src.height, src.width)
        if self._src is not None:
            f = self._src.get_image()
            if f is not None:
                self.last_index = self._src.index
            return self._scaled(f)
        n = len(self._frames) if self._frames is not None else len(self._files)
        if self._i >= n:
            return None
        if self._frames is not None:
            f = np.ascontiguousarray(self._frames[self._i])
        else:
            from PIL import Image

            f = np.asarray(Image.open(self._files[self._i]).convert("RGB"))
        self.last_index = self._i
        self._i += self.world
        return self._scaled(f)

    # ---- sink ------------------------------------------------------------------------------------------
    def _shard_path(self, rank: int) -> str:
        return self.write_path if self.world == 1 else f"{self.write_path[:-4]}.rank{rank}of{self.world}{self.write_path[-4:]}"

    def _own_count(self) -> Optional[int]:
        return None if self.total_frames is None else len(range(self.rank, self.total_frames, self.world))

    def render(self, frame: np.ndarray, *, index: Optional[int] = None) -> None:
        """renderers/video.py:118-142 (write the frame).  `index` = the frame's GLOBAL stream index; by default frames are
        taken to arrive in this rank's stream order (rank, rank + world, ...).  A .y4m sink also takes flat I420 payloads of the
        source's size, and writes its frames in this rank's stream order (one shard per rank when world > 1)."""
        if index is None:
            index = self.rank + self.frames_written * self.world
        if self.write_path:
            if self.write_pix_fmt is not None:
                self._render_raw(frame, index)
            elif is_y4m(self.write_path):
                self._render_y4m(frame, index)
            elif self.write_path.endswith(".npy"):
                row = (index - self.rank) // self.world
                if (index - self.rank) % self.world or row < 0:
                    raise ValueError(f"frame {index} does not belong to rank {self.rank} of {self.world}")
                if self._sink is None or row >= self._sink_rows:
                    self._grow_sink(frame, row)
                self._sink[row] = frame
            else:
                from PIL import Image

                Image.fromarray(frame).save(os.path.join(self.write_path, f"frame_{index:06d}.png"))
        self.frames_written += 1

    def _render_y4m(self, frame: np.ndarray, index: int) -> None:
        if index != self.rank + self.frames_written * self.world:
            raise ValueError(f"frame {index}: a .y4m sink is written in stream order; rank {self.rank} of {self.world} expects frame "
                             f"{self.rank + self.frames_written * self.world}")
        frame = np.asarray(frame)
        if frame.ndim == 3:
            if frame.dtype != np.uint8 or frame.shape[2] != 3:
                raise ValueError(f"a .y4m sink takes RGB uint8 HxWx3 frames or I420 payloads, got {frame.dtype} {frame.shape}")
            H, W = frame.shape[:2]
            payload = self.encode.arrays(frame)
        elif frame.ndim == 1 and frame.dtype == np.uint8:
            if self._y4m_out is None and self._y4m is None and self._sink_hw is None:
                raise ValueError("an I420 payload names no frame size: render an RGB frame first, read from a .y4m, or call set_output_size()")
            if self._y4m_out is not None or (self.scale is None and self._sink_hw is None):
                hdr = self._y4m_out.header if self._y4m_out is not None else self._y4m.header
                H, W = hdr.height, hdr.width
            else:
                H, W = self.sink_hw  # payloads arrive scaled, or at the size set_output_size() named
            payload = frame
        else:
            raise ValueError(f"a .y4m sink takes RGB uint8 HxWx3 frames or flat uint8 I420 payloads, got {frame.dtype} {frame.shape}")
        if self._y4m_out is None:
            self._open_y4m_sink(H, W)
        self._y4m_out.write(payload)

    def _render_raw(self, frame: np.ndarray, index: int) -> None:
        """A raw sink takes RGB uint8 HxWx3 frames (encoded on the device) or flat payloads in write_pix_fmt, in stream order."""
        if index != self.rank + self.frames_written * self.world:
            raise ValueError(f"frame {index}: a raw video sink is written in stream order; rank {self.rank} of {self.world} expects frame "
                             f"{self.rank + self.frames_written * self.world}")
        frame = np.asarray(frame)
        if frame.ndim == 3 and frame.dtype == np.uint8 and frame.shape[2] == 3:
            H, W = frame.shape[:2]
            payload = self.encode.arrays(frame)
        elif frame.ndim == 1 and frame.dtype == np.uint8:
            if self._raw_out is None and self._sink_hw is None and (self._raw is None or self.pix_fmt != self.write_pix_fmt):
                raise ValueError(f"a {self.write_pix_fmt} payload names no frame size: render an RGB frame first, read raw video in that "
                                 "format, or call set_output_size()")
            H, W = (self._raw_out.height, self._raw_out.width) if self._raw_out is not None else self.sink_hw  # payloads arrive scaled
            payload = frame
        else:
            raise ValueError(f"a raw video sink takes RGB uint8 HxWx3 frames or flat uint8 {self.write_pix_fmt} payloads, got {frame.dtype} {frame.shape}")
        if self._raw_out is None:
            self._open_raw_sink(H, W)
        self._raw_out.write(payload)

    def _open_raw_sink(self, H: int, W: int) -> None:
        from .rawvideo import RawVideoWriter

        self._raw_out = RawVideoWriter(self._shard_path(self.rank), self.write_pix_fmt, W, H)
        self._merge_size = (W, H)

    def _open_y4m_sink(self, H: int, W: int) -> None:
        """Create the .y4m sink (this rank's shard when world > 1) and write its header."""
        from .y4m import Y4MWriter, default_header

        if self._y4m is not None:  # echo the source's header: rate, aspect, unknown tags; the range this sink encodes with
            hdr = self._y4m.header.with_size(W, H)
            hdr = hdr.replaced("XCOLORRANGE=", "FULL" if self.yuv_range == "full" else ("LIMITED" if hdr.tag("XCOLORRANGE=") else None))
        else:
            hdr = default_header(W, H, fps=self.fps, full_range=self.yuv_range == "full")
        self._y4m_out = Y4MWriter(self._shard_path(self.rank), hdr)

    def _grow_sink(self, frame: np.ndarray, row: int) -> None:
        """Create the shard on first use (sized from the source's frame count when it is known); a stream of unknown length
        doubles the mapping (old rows are copied once per doubling, on disk)."""
        want = self._own_count() or 0
        rows = max(want, row + 1, 2 * self._sink_rows, 1)
        path = self._shard_path(self.rank)
        new = np.lib.format.open_memmap(path + ".tmp" if self._sink is not None else path, mode="w+", dtype=frame.dtype, shape=(rows,) + frame.shape)
        if self._sink is not None:
            new[: self._sink_rows] = self._sink[: self._sink_rows]
            new.flush()
            del self._sink
            os.replace(path + ".tmp", path)
            new = np.load(path, mmap_mode="r+")
        self._sink, self._sink_rows = new, rows

    def flush(self) -> None:
        """Everything rendered so far is on disk as a well-formed .npy (a mapping sized for more frames than arrived is
        trimmed to what was written); rendering may continue afterwards."""
        if self._y4m_out is not None:
            self._y4m_out.flush()
        if self._raw_out is not None:
            self._raw_out.flush()
        if self._sink is None:
            return
        self._sink.flush()
        written, rows, path = self.frames_written, self._sink_rows, self._shard_path(self.rank)
        if written < rows:
            shape, dtype = self._sink.shape[1:], self._sink.dtype
            tmp = np.lib.format.open_memmap(path + ".tmp", mode="w+", dtype=dtype, shape=(written,) + shape)
            tmp[:] = self._sink[:written]
            tmp.flush()
            del tmp
            self._sink = None
            os.replace(path + ".tmp", path)
            self._sink, self._sink_rows = np.load(path, mmap_mode="r+"), written

    def close(self) -> None:
        self.flush()
        self._sink = None
        self._src = self._frames = None
        if self._y4m_out is None and self._y4m is not None and is_y4m(self.write_path) and self.write_pix_fmt is None:
            # no frame was rendered: the sink is still a valid (empty) stream, its header at the source's size
            self._open_y4m_sink(*self.sink_hw)
        if self._y4m_out is not None:
            self._y4m_out.close()
            self._y4m_out = None
        if self._y4m is not None:
            self._y4m.close()
            self._y4m = None
        if self._raw_out is None and self._raw is not None and self.write_pix_fmt is not None:
            self._open_raw_sink(*self.sink_hw)  # no frame was rendered: an empty file, not a missing one
        if self._raw_out is not None:
            self._raw_out.close()
            self._raw_out = None
        if self._raw is not None:
            self._raw.close()
            self._raw = None

    def merge_shards(self) -> Optional[str]:
        """Rank 0, after every rank has flushed/closed its shard (run_video calls it behind the closing collective): interleave
        <write_path>.rank<r>of<world>.npy (.y4m) into the one ordered stream <write_path>, frame i from shard i mod world."""
        if self.write_path and self.write_pix_fmt is not None:
            return self._merge_raw_shards() if self.world > 1 else self.write_path
        if self.write_path and is_y4m(self.write_path) and self.world > 1:
            return self._merge_y4m_shards()
        if not (self.write_path and self.write_path.endswith(".npy")) or self.world == 1:
            return self.write_path
        shards = [np.load(self._shard_path(r), mmap_mode="r") if os.path.exists(self._shard_path(r)) else None for r in range(self.world)]
        have = [s for s in shards if s is not None]
        if not have:
            return None
        n = sum(len(s) for s in have)
        out = np.lib.format.open_memmap(self.write_path, mode="w+", dtype=have[0].dtype, shape=(n,) + have[0].shape[1:])
        for r, s in enumerate(shards):
            if s is not None:
                idx = np.arange(r, r + len(s) * self.world, self.world)
                if len(idx) and idx[-1] >= n:
                    raise ValueError("shards are not a round-robin partition of one stream")
                for k, i in enumerate(idx):  # frame by frame: bounded memory
                    out[i] = s[k]
        out.flush()
        del out, shards, have
        for r in range(self.world):
            if os.path.exists(self._shard_path(r)):
                os.remove(self._shard_path(r))
        return self.write_path

    def _merge_raw_shards(self) -> Optional[str]:
        """Raw shards carry no header: every one holds whole frames of one size, which the first non-empty shard's writer knew.
        The frame size comes from this renderer's source size, else from `size`."""
        paths = [self._shard_path(r) for r in range(self.world)]
        if self._merge_size is None:
            raise ValueError("merging raw video shards needs the frame size: render a frame first, or pass size=(W, H)")
        W, H = self._merge_size
        from .rawvideo import RawVideoReader, RawVideoWriter

        shards = [RawVideoReader(p, self.write_pix_fmt, W, H) if os.path.exists(p) else None for p in paths]
        have = [s for s in shards if s is not None]
        if not have:
            return None
        n = sum(s.total_frames for s in have)
        counts = [0 if s is None else s.total_frames for s in shards]
        if counts != [len(range(r, n, self.world)) for r in range(self.world)]:
            raise ValueError(f"shards of {counts} frames are not a round-robin partition of one stream")
        out = RawVideoWriter(self.write_path, self.write_pix_fmt, W, H)
        try:
            for i in range(n):  # frame by frame: bounded memory
                out.write(shards[i % self.world].read())
        finally:
            out.close()
            for s in have:
                s.close()
        for p in paths:
            if os.path.exists(p):
                os.remove(p)
        return self.write_path

    def _merge_y4m_shards(self) -> Optional[str]:
        from .y4m import Y4MReader, Y4MWriter

        paths = [self._shard_path(r) for r in range(self.world)]
        shards = [Y4MReader(p) if os.path.exists(p) else None for p in paths]
        have = [s for s in shards if s is not None]
        if not have:
            return None
        n = sum(s.total_frames for s in have)
        counts = [0 if s is None else s.total_frames for s in shards]
        if counts != [len(range(r, n, self.world)) for r in range(self.world)]:
            raise ValueError(f"shards of {counts} frames are not a round-robin partition of one stream")
        out = Y4MWriter(self.write_path, have[0].header)
        try:
            for i in range(n):  # frame by frame: bounded memory
                out.write(shards[i % self.world].read())
        finally:
            out.close()
            for s in have:
                s.close()
        for p in paths:
            if os.path.exists(p):
                os.remove(p)
        return self.write_path

    # ---- split compare ---------------------------------------------------------------------------------
    def make_split_frame(self, original: np.ndarray, modified: np.ndarray, *, left_label: str = "Original",
                         right_label: str = "Transformed", draw_seam: bool = True) -> np.ndarray:
        return split_compose(original, modified, draw_seam, left_label=left_label, right_label=right_label)

    def render_split_compare(self, original: np.ndarray, modified: np.ndarray, *, left_label: str = "Original",
                             right_label: str = "Transformed", draw_seam: bool = True) -> None:
        self.render(self.make_split_frame(original, modified, left_label=left_label, right_label=right_label, draw_seam=draw_seam))
