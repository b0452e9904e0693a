"""MI355X-native render hot path of MobileRT (TiagoMSSantos/MobileRayTracer).

Python mirror of the reference's native surface for this path:

* ``Config``            — ``MobileRT::Config`` (app/MobileRT/Config.hpp:12-83)
* ``Renderer``          — ``MobileRT::Renderer`` (app/MobileRT/Renderer.hpp:41-63) as built by
                          ``work_thread`` (app/System_dependent/Native/C_wrapper.cpp:36-211):
                          the constructor assembles scene + shader + BVH + camera, then
                          ``render_frame`` / ``stop_render`` / ``get_sample`` /
                          ``get_total_casted_rays`` keep the reference's meaning.
* ``ray_trace``         — ``RayTrace(Config&, bool)`` (C_wrapper.cpp:268-290).

Everything computes in the HIP kernels of ``libmobilert_amd.so``; there is no CPU path.
"""
import contextlib
import ctypes
import dataclasses
import threading
import time
from typing import List, Optional

import numpy as np

from . import _native

SHADER_WHITTED = 1      # C_wrapper.cpp:155
SHADER_PATH_TRACER = 2  # C_wrapper.cpp:162
ACC_BVH = 3             # Shader.hpp:20-24
RAY_DEPTH_MAX = 6       # Constants.hpp:45


@dataclasses.dataclass
class Config:
    """MobileRT::Config plus the GPU-only knobs of mrt_config."""
    width: int = 256
    height: int = 256
    threads: int = 1
    shader: int = SHADER_WHITTED
    sceneIndex: int = 0
    samplesPixel: int = 1
    samplesLight: int = 1
    repeats: int = 1
    accelerator: int = ACC_BVH
    printStdOut: bool = False
    objFilePath: str = ""
    mtlFilePath: str = ""
    camFilePath: str = ""
    bitmap: Optional[np.ndarray] = None
    maxDepth: int = RAY_DEPTH_MAX
    rankIndex: int = 0
    rankCount: int = 1
    device: int = -1
    cull: int = 3
    maxPathsPerPass: int = 0
    progressive: int = 0
    # a device group: one screen-tile shard per listed HIP device, assembled on devices[0]
    # (mrt_config.devices; empty or one entry: a single GPU, `device`)
    devices: List[int] = dataclasses.field(default_factory=list)

    def to_c(self):
        c = _native.MrtConfig()
        for f in ("width", "height", "threads", "shader", "sceneIndex", "samplesPixel", "samplesLight",
                  "repeats", "accelerator", "maxDepth", "rankIndex", "rankCount", "device", "cull",
                  "maxPathsPerPass", "progressive"):
            setattr(c, f, int(getattr(self, f)))
        c.printStdOut = int(bool(self.printStdOut))
        self._keep = [s.encode() for s in (self.objFilePath, self.mtlFilePath, self.camFilePath)]
        c.objFilePath, c.mtlFilePath, c.camFilePath = self._keep
        if len(self.devices) > 1:
            self._keep_devices = (ctypes.c_int32 * len(self.devices))(*[int(d) for d in self.devices])
            c.devices = self._keep_devices
            c.deviceCount = len(self.devices)
        return c


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


class Renderer:
    def __init__(self, config: Config):
        self._lib = _native.lib()
        self.config = config
        handle = ctypes.c_void_p()
        _native.check(self._lib.mrt_create(ctypes.byref(config.to_c()), ctypes.byref(handle)))
        self._h = handle

    # -- reference Renderer surface ------------------------------------------------------
    def render_frame(self, bitmap: np.ndarray, num_threads: int = 1) -> None:
        """Renderer::renderFrame(int32_t *bitmap, int32_t numThreads); numThreads is unused."""
        del num_threads
        assert bitmap.dtype == np.int32 and bitmap.size == self.config.width * self.config.height
        assert bitmap.flags["C_CONTIGUOUS"]
        _native.check(self._lib.mrt_render_frame(self._h, _ptr(bitmap)))

    def render_frame_device(self, d_bitmap: int = 0, d_packed: int = 0, stream: int = 0) -> None:
        """Frame into device memory (pointers as ints, e.g. torch ``data_ptr()``)."""
        _native.check(self._lib.mrt_render_frame_device(
            self._h, ctypes.c_void_p(d_bitmap or None), ctypes.c_void_p(d_packed or None),
            ctypes.c_void_p(stream or None)))

    # -- batches of views ----------------------------------------------------------------
    @staticmethod
    def _views(cameras):
        """``cameras``: a sequence of set_camera's tuples (kind, position, look_at, up, a, b)."""
        views = (_native.MrtView * max(1, len(cameras)))()
        for v, (kind, position, look_at, up, a, b) in zip(views, cameras):
            v.kind = int(kind)
            v.position[:] = [float(x) for x in position]
            v.lookAt[:] = [float(x) for x in look_at]
            v.up[:] = [float(x) for x in up]
            v.a, v.b = float(a), float(b)
        return views

    def render_views(self, cameras, bitmaps: np.ndarray) -> None:
        """mrt_render_views: one frame per camera in one submission, view v into ``bitmaps[v]`` (C-contiguous
        int32 of shape (K, width*height)), bit-equal to set_camera + render_frame per view; the
        renderer's own camera is unchanged."""
        assert bitmaps.dtype == np.int32 and bitmaps.flags["C_CONTIGUOUS"]
        assert bitmaps.shape == (len(cameras), self.config.width * self.config.height)
        _native.check(self._lib.mrt_render_views(self._h, self._views(cameras), len(cameras), _ptr(bitmaps)))

    def render_views_device(self, cameras, d_bitmaps: int = 0, d_packed: int = 0, stream: int = 0) -> None:
        """mrt_render_views_device: the batch into device memory (pointers as ints, e.g. a torch int32
        tensor's ``data_ptr()``): ``d_bitmaps`` K x (width*height), ``d_packed`` K x pixelSlots."""
        _native.check(self._lib.mrt_render_views_device(
            self._h, self._views(cameras), len(cameras), ctypes.c_void_p(d_bitmaps or None),
            ctypes.c_void_p(d_packed or None), ctypes.c_void_p(stream or None)))

    def unpack_gathered(self, d_gathered: int, d_bitmap: int, stream: int = 0) -> None:
        _native.check(self._lib.mrt_unpack_gathered(self._h, ctypes.c_void_p(d_gathered),
                                                     ctypes.c_void_p(d_bitmap), ctypes.c_void_p(stream or None)))

    def stop_render(self) -> None:
        _native.check(self._lib.mrt_stop_render(self._h))

    def get_sample(self) -> int:
        return int(self._lib.mrt_get_sample(self._h))

    def get_total_casted_rays(self) -> int:
        return int(self._lib.mrt_get_total_casted_rays(self._h))

    # -- extras --------------------------------------------------------------------------
    def scene_info(self) -> dict:
        info = _native.MrtSceneInfo()
        _native.check(self._lib.mrt_get_scene_info(self._h, ctypes.byref(info)))
        return {f: getattr(info, f) for f, _ in info._fields_}

    def set_profiling(self, timing: bool = False, counting: bool = False) -> None:
        _native.check(self._lib.mrt_set_profiling(self._h, int(timing) | (2 * int(counting))))

    def set_tuning(self, key: int, value: int) -> None:
        """A/B knobs: 1 = trace walk (0 reference, 1 default), 2 = t-cull mode (0 none, 1 fast -
        inexact on grazing inputs, 2 certified, 3 exact: the default), 3 = shadow rays on their own
        stream, 5 = shadow-walk child order (0 near first, 1 far first),
        6 = shadow-walk grid percent (0 auto), 7 = no walk for the depth-capped last level, 8 = tail
        donation (idle lanes of a level's tail walk subtrees of their wave's rays), 9 = refill
        threshold of the walk waves, 10 = lean k_shade instantiation, 11 = k_shade workgroups per CU,
        16 = the camera rays' packet walk (cull modes 0 and 3; refused when the walk tree needs a
        deeper stack than the packet walk's), 17 = level 1 fused (camera rays generated,
        packet-walked and shaded in one launch), 19-23 = the tile kernel and its knobs, 27 = the
        last shadow walk on the render stream, 37 = byte budget of the wavefront queues in MiB
        (0 automatic), 38 = the first allocation's deeper levels in percent of level 1 (200),
        39 = slack slots per queue segment (3072); 37-39 reallocate the queues from the next frame.
        Results are identical for every value, except key 2 = 1 (documented inexact)."""
        _native.check(self._lib.mrt_set_tuning(self._h, key, value))

    def set_camera(self, kind: int, position, look_at, up, a: float, b: float) -> None:
        """mrt_set_camera: kind 0 Perspective(position, lookAt, up, hFov, vFov in degrees), 1
        Orthographic(position, lookAt, up, sizeH, sizeV) (Perspective.cpp / Orthographic.cpp)."""
        vec = lambda v: (ctypes.c_float * 3)(*[float(x) for x in v])  # noqa: E731
        _native.check(self._lib.mrt_set_camera(self._h, kind, vec(position), vec(look_at), vec(up), a, b))

    def set_pixel_sampler(self, kind: int, value: float = 0.5) -> None:
        """mrt_set_pixel_sampler: 0 Constant(value), 1 StaticHaltonSeq (the Renderer's pixel sampler)."""
        _native.check(self._lib.mrt_set_pixel_sampler(self._h, kind, value))

    def set_max_point(self, max_point) -> None:
        """mrt_set_max_point: DepthMap's maxPoint."""
        _native.check(self._lib.mrt_set_max_point(self._h, (ctypes.c_float * 3)(*[float(x) for x in max_point])))

    def get_tuning(self, key: int) -> int:
        v = ctypes.c_int32(0)
        _native.check(self._lib.mrt_get_tuning(self._h, key, ctypes.byref(v)))
        return v.value

    def wave_log(self):
        """Counting mode: the last frame's per-wave log, uint64 [2 (closest, any-hit), 16 levels,
        8192 waves, 4 (start, end in 100 MHz ticks, rays fetched, child records fetched)]."""
        n = int(self._lib.mrt_wave_log(self._h, None))
        out = np.zeros(n, np.uint64)
        _native.check(0 if self._lib.mrt_wave_log(self._h, out.ctypes.data_as(ctypes.c_void_p)) >= 0 else -1)
        return out.reshape(2, 16, 8192, 4)

    def frame_stats(self) -> dict:
        s = _native.MrtFrameStats()
        _native.check(self._lib.mrt_get_frame_stats(self._h, ctypes.byref(s)))
        out = {f: getattr(s, f) for f, _ in s._fields_}
        out["levelRays"] = list(s.levelRays)
        out["levelShadowRays"] = list(s.levelShadowRays)
        out["levelTraceMs"] = list(s.levelTraceMs)
        out["levelShadowMs"] = list(s.levelShadowMs)
        for k in ("levelNodeRecords", "levelTriTests", "levelLeafRecords", "levelShadedVertices", "walkPhases",
                  "packetWaveRecords"):
            out[k] = list(getattr(s, k))
        return out

    def queue_info(self) -> dict:
        """mrt_get_queue_info: the wavefront queues' plan (chunkSlots, passes per sample set, queueBytes,
        budgetBytes, replans since creation and during the last frame, worstCase, per depth rayCap /
        shadowCap) and what the last pass asked of them (requestedRays / requestedShadows)."""
        q = _native.MrtQueueInfo()
        _native.check(self._lib.mrt_get_queue_info(self._h, ctypes.byref(q), ctypes.sizeof(q)))
        out = {f: getattr(q, f) for f, _ in q._fields_}
        for k in ("rayCap", "shadowCap", "requestedRays", "requestedShadows"):
            out[k] = list(getattr(q, k))
        return out

    def frame_rays(self):
        """(walkedRays, shadowRays) of the last frame: frame_stats()'s two ray counts without building
        its dict (a per-frame call in bench.py's timed loop)."""
        s = getattr(self, "_rays_buf", None)
        if s is None:
            s = self._rays_buf = _native.MrtFrameStats()
        _native.check(self._lib.mrt_get_frame_stats(self._h, ctypes.byref(s)))
        return s.walkedRays, s.shadowRays

    def primary_hits(self):
        """(kind, index, t) per pixel, index in the scene's input order (config C2)."""
        n = self.config.width * self.config.height
        kind = np.empty(n, np.int32)
        index = np.empty(n, np.int32)
        t = np.empty(n, np.float32)
        _native.check(self._lib.mrt_primary_hits(self._h, _ptr(kind), _ptr(index), _ptr(t)))
        return kind, index, t

    def trace_rays(self, orig, dirs, dist=None, src=None, any_hit=False):
        """Arbitrary rays through the trace kernels (current walk / cull): closest hit
        (kind, input index, t) per ray, or with any_hit the shadow test within dist
        (kind = occluded).  src: None or (n, 2) int32 (kind, input index) source primitives."""
        o = np.ascontiguousarray(orig, np.float32)
        d = np.ascontiguousarray(dirs, np.float32)
        n = len(o)
        ds = np.ascontiguousarray(dist if dist is not None else np.zeros(n), np.float32)
        sp = None if src is None else np.ascontiguousarray(src, np.int32)
        k, i, t = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float32)
        _native.check(self._lib.mrt_trace_rays(self._h, _ptr(o), _ptr(d), _ptr(ds), None if sp is None else _ptr(sp),
                                               n, int(any_hit), _ptr(k), _ptr(i), _ptr(t)))
        return k, i, t

    # -- ray queries ---------------------------------------------------------------------
    def cast_rays_device(self, d_orig: int, d_dir: int, n: int, *, d_dist: int = 0, d_src: int = 0,
                         orig_stride: int = 3, dir_stride: int = 3, any_hit: bool = False, d_kind: int = 0,
                         d_index: int = 0, d_t: int = 0, stream: int = 0) -> None:
        """mrt_cast_rays_device: ``n`` rays resident in device memory through the walks, the results
        into device memory (pointers as ints, e.g. torch ``data_ptr()``; strides in floats).  Closest
        hit: ``d_kind`` / ``d_index`` int32 and ``d_t`` float32 per ray, as trace_rays; ``any_hit``:
        ``d_kind`` = occluded within ``d_dist[i]``, nothing else written.  ``d_src``: (n, 2) int32
        (kind, input index) of the primitive each ray leaves, or 0.  Outputs passed as 0 are not
        written.  The work is ordered after ``stream``'s earlier work and before its later work, and
        the call returns after enqueuing it; ``stream`` 0 is the renderer's own stream."""
        batch = _native.MrtRayBatch(d_orig or None, d_dir or None, d_dist or None, d_src or None,
                                    int(orig_stride), int(dir_stride), int(n))
        _native.check(self._lib.mrt_cast_rays_device(
            self._h, ctypes.byref(batch), int(bool(any_hit)), ctypes.c_void_p(d_kind or None),
            ctypes.c_void_p(d_index or None), ctypes.c_void_p(d_t or None), ctypes.c_void_p(stream or None)))

    def cast_rays(self, orig, dirs, dist=None, src=None, any_hit=False):
        """cast_rays_device for torch tensors on the renderer's device: ``orig`` / ``dirs`` float32 of
        shape (n, >= 3); ``dist`` float32 (n,), ``src`` int32 (n, 2).  Rows that are at least 3
        floats apart with adjacent columns are read in place (a slice of a wider array: the strides
        are taken from the tensors); any other layout - a broadcast ``expand`` of one origin, whose
        rows are 0 apart, transposed columns - is made contiguous first.  Returns (kind, index, t),
        or with ``any_hit`` the occlusion flags (int32), allocated and ordered on torch's current
        stream; nothing is copied to the host and nothing waits for the device.  An empty batch
        returns empty tensors (the C entry point itself takes 1 .. 2^31 - 1 rays).  Raises
        ValueError for a tensor that is not on the renderer's GPU or has another shape."""
        import torch

        device, n, orig, orig_stride, dirs, dir_stride = self._ray_tensors(orig, dirs)
        if any_hit:
            if dist is None:
                raise ValueError("any_hit needs dist")
            if dist.device != device or dist.shape != (n,):
                raise ValueError("dist: a tensor of shape (%d,) on %s" % (n, device))
            dist = dist.to(torch.float32).contiguous()
        if src is not None:
            if src.device != device or src.shape != (n, 2):
                raise ValueError("src: a tensor of shape (%d, 2) on %s" % (n, device))
            src = src.to(torch.int32).contiguous()
        kind = torch.empty(n, dtype=torch.int32, device=device)
        index = None if any_hit else torch.empty(n, dtype=torch.int32, device=device)
        t = None if any_hit else torch.empty(n, dtype=torch.float32, device=device)
        if n == 0:
            return kind if any_hit else (kind, index, t)
        with self._query_stream_of(device) as stream:
            self.cast_rays_device(orig.data_ptr(), dirs.data_ptr(), n, d_dist=dist.data_ptr() if any_hit else 0,
                                  d_src=src.data_ptr() if src is not None else 0, orig_stride=orig_stride,
                                  dir_stride=dir_stride, any_hit=any_hit, d_kind=kind.data_ptr(),
                                  d_index=0 if any_hit else index.data_ptr(), d_t=0 if any_hit else t.data_ptr(),
                                  stream=stream)
        return kind if any_hit else (kind, index, t)

    def _ray_tensors(self, orig, dirs):
        """The tensor handling of cast_rays / shade_rays: (device, n, orig, orig_stride, dirs,
        dir_stride), the strides in floats and never 0, which the C entry points take for 'packed'
        (rows 3 apart).  ValueError for a tensor off the renderer's GPU or of another shape."""
        import torch

        device = orig.device
        want = self.config.device if not self.config.devices else -1
        if not orig.is_cuda or (want >= 0 and device.index != want):
            raise ValueError("orig: a tensor on the renderer's GPU (it is on %s)" % device)
        n = orig.shape[0] if orig.dim() == 2 else -1

        def rows(a, name):
            if a.device != device or a.dtype != torch.float32 or a.dim() != 2 or a.shape[0] != n or a.shape[1] < 3:
                raise ValueError("%s: a float32 tensor of shape (%d, >= 3) on %s" % (name, n, device))
            if a.stride(1) != 1 or (n > 1 and a.stride(0) < 3):
                a = a[:, :3].contiguous()
            return a, (a.stride(0) if n > 1 else 3)

        orig, orig_stride = rows(orig, "orig")
        dirs, dir_stride = rows(dirs, "dirs")
        return device, n, orig, orig_stride, dirs, dir_stride

    @contextlib.contextmanager
    def _query_stream_of(self, device):
        """The stream handle a query on torch's current stream is given.  Handle 0 would mean the
        renderer's own stream, which is not ordered against torch's null stream: from there the query
        goes through a stream of this renderer's, joined to the null stream by torch on both sides
        (events only; nothing waits on the host)."""
        import torch

        current = torch.cuda.current_stream(device)
        via = current
        if current.cuda_stream == 0:
            via = getattr(self, "_query_stream", None)
            if via is None:
                via = self._query_stream = torch.cuda.Stream(device)
            via.wait_stream(current)
        try:
            yield via.cuda_stream
        finally:
            if via is not current:
                current.wait_stream(via)

    # -- surface records -----------------------------------------------------------------
    HIT_FIELDS = tuple(name for name, _, _ in _native.HIT_FIELDS)

    def cast_hits_device(self, d_orig: int, d_dir: int, n: int, *, d_src: int = 0, orig_stride: int = 3,
                         dir_stride: int = 3, stream: int = 0, out_size: Optional[int] = None, **outputs: int) -> None:
        """mrt_cast_hits_device: the closest hit of ``n`` rays resident in device memory as surface
        records.  ``outputs``: ``d_kind``, ``d_index``, ``d_t``, ``d_bary``, ``d_point``, ``d_normal``,
        ``d_texCoord``, ``d_material``, ``d_kd``, ``d_ks``, ``d_kt``, ``d_le``, ``d_ior`` - device
        pointers as ints to packed arrays (mrt_hit_records), 0 or absent: not wanted.  ``out_size``:
        the bytes of the structure the library may read (None: all of it).  Rays, ``d_src``, strides
        and ``stream`` as for cast_rays_device."""
        rec = _native.MrtHitRecords()
        for key, value in outputs.items():
            if not key.startswith("d_") or key[2:] not in self.HIT_FIELDS:
                raise TypeError("cast_hits_device: unknown output %r" % key)
            setattr(rec, key[2:], value or None)
        batch = _native.MrtRayBatch(d_orig or None, d_dir or None, None, d_src or None, int(orig_stride),
                                    int(dir_stride), int(n))
        size = ctypes.sizeof(rec) if out_size is None else int(out_size)
        _native.check(self._lib.mrt_cast_hits_device(self._h, ctypes.byref(batch), ctypes.byref(rec), size,
                                                     ctypes.c_void_p(stream or None)))

    def cast_hits(self, orig, dirs, src=None, fields=None):
        """cast_hits_device for torch tensors on the renderer's device, with cast_rays' handling of
        ``orig`` / ``dirs`` / ``src`` and its stream joining.  Returns a dict of tensors, one per name
        in ``fields`` (None: all of ``Renderer.HIT_FIELDS``): int32 ``kind`` / ``index`` / ``material``
        of shape (n,), float32 ``t`` / ``ior`` (n,), ``bary`` / ``texCoord`` (n, 2) and ``point`` /
        ``normal`` / ``kd`` / ``ks`` / ``kt`` / ``le`` (n, 3), allocated and ordered on torch's current
        stream.  An empty batch returns empty tensors."""
        import torch

        device, n, orig, orig_stride, dirs, dir_stride = self._ray_tensors(orig, dirs)
        fields = self.HIT_FIELDS if fields is None else tuple(fields)
        if not fields or any(f not in self.HIT_FIELDS for f in fields):
            raise ValueError("fields: at least one of %s" % (self.HIT_FIELDS,))
        if src is not None:
            if src.device != device or src.shape != (n, 2):
                raise ValueError("src: a tensor of shape (%d, 2) on %s" % (n, device))
            src = src.to(torch.int32).contiguous()
        out = {}
        for name, dtype, width in _native.HIT_FIELDS:
            if name in fields:
                out[name] = torch.empty(n if width == 1 else (n, width), dtype=getattr(torch, dtype), device=device)
        if n == 0:
            return out
        with self._query_stream_of(device) as stream:
            self.cast_hits_device(orig.data_ptr(), dirs.data_ptr(), n, d_src=src.data_ptr() if src is not None else 0,
                                  orig_stride=orig_stride, dir_stride=dir_stride, stream=stream,
                                  **{"d_" + name: x.data_ptr() for name, x in out.items()})
        return out

    # -- multi-hit queries ---------------------------------------------------------------
    MULTI_HIT_FIELDS = tuple(name for name, _, _ in _native.MULTI_HIT_FIELDS)

    def cast_multi_hits_device(self, d_orig: int, d_dir: int, n: int, k: int, *, d_dist: int = 0, d_src: int = 0,
                               orig_stride: int = 3, dir_stride: int = 3, d_count: int = 0, d_kind: int = 0,
                               d_index: int = 0, d_t: int = 0, d_bary: int = 0, stream: int = 0,
                               out_size: Optional[int] = None) -> None:
        """mrt_cast_multi_hits_device: the first ``k`` (1 .. 16) hits along each of ``n`` rays resident in
        device memory, in order, and each ray's hit count.  ``d_count`` (n int32), ``d_kind`` / ``d_index``
        (n x k int32), ``d_t`` (n x k float32), ``d_bary`` (n x k x 2 float32): device pointers as ints to
        packed arrays (mrt_multi_hits), 0: not wanted.  ``d_dist``: the rays' interval ends (n float32),
        0: RayLengthMax.  ``out_size``: the bytes of the structure the library may read (None: all of
        it).  Rays, ``d_src``, strides and ``stream`` as for cast_rays_device."""
        out = _native.MrtMultiHits(d_count or None, d_kind or None, d_index or None, d_t or None, d_bary or None)
        batch = _native.MrtRayBatch(d_orig or None, d_dir or None, d_dist or None, d_src or None, int(orig_stride),
                                    int(dir_stride), int(n))
        size = ctypes.sizeof(out) if out_size is None else int(out_size)
        _native.check(self._lib.mrt_cast_multi_hits_device(self._h, ctypes.byref(batch), int(k), ctypes.byref(out), size,
                                                           ctypes.c_void_p(stream or None)))

    def cast_multi_hits(self, orig, dirs, k: int, dist=None, src=None, fields=None):
        """cast_multi_hits_device for torch tensors on the renderer's device, with cast_rays' handling of
        ``orig`` / ``dirs`` / ``src`` and its stream joining; ``dist`` float32 (n,) or None (RayLengthMax).
        Returns a dict of tensors, one per name in ``fields`` (None: all of ``Renderer.MULTI_HIT_FIELDS``):
        int32 ``count`` (n,), int32 ``kind`` / ``index`` (n, k), float32 ``t`` (n, k) and ``bary`` (n, k, 2),
        allocated and ordered on torch's current stream.  An empty batch returns empty tensors."""
        import torch

        device, n, orig, orig_stride, dirs, dir_stride = self._ray_tensors(orig, dirs)
        k = int(k)
        if not 1 <= k <= _native.MULTI_HITS_MAX:
            raise ValueError("k: 1 .. %d" % _native.MULTI_HITS_MAX)
        fields = self.MULTI_HIT_FIELDS if fields is None else tuple(fields)
        if not fields or any(f not in self.MULTI_HIT_FIELDS for f in fields):
            raise ValueError("fields: at least one of %s" % (self.MULTI_HIT_FIELDS,))
        if dist is not None:
            if dist.device != device or dist.shape != (n,):
                raise ValueError("dist: a tensor of shape (%d,) on %s" % (n, device))
            dist = dist.to(torch.float32).contiguous()
        if src is not None:
            if src.device != device or src.shape != (n, 2):
                raise ValueError("src: a tensor of shape (%d, 2) on %s" % (n, device))
            src = src.to(torch.int32).contiguous()
        out = {}
        for name, dtype, width in _native.MULTI_HIT_FIELDS:
            if name in fields:
                shape = (n,) if width == 0 else (n, k) if width == 1 else (n, k, width)
                out[name] = torch.empty(shape, dtype=getattr(torch, dtype), device=device)
        if n == 0:
            return out
        with self._query_stream_of(device) as stream:
            self.cast_multi_hits_device(orig.data_ptr(), dirs.data_ptr(), n, k,
                                        d_dist=dist.data_ptr() if dist is not None else 0,
                                        d_src=src.data_ptr() if src is not None else 0, orig_stride=orig_stride,
                                        dir_stride=dir_stride, stream=stream,
                                        **{"d_" + name: x.data_ptr() for name, x in out.items()})
        return out

    # -- nearest-point queries -----------------------------------------------------------
    NEAREST_FIELDS = tuple(name for name, _, _ in _native.NEAREST_FIELDS)

    def nearest_points_device(self, d_point: int, n: int, /, *, d_dist: int = 0, d_src: int = 0, stride: int = 3,
                              stream: int = 0, out_size: Optional[int] = None, **outputs: int) -> None:
        """mrt_nearest_points_device: the nearest surface to each of ``n`` points resident in device
        memory (point i's xyz at ``d_point`` + i * ``stride`` floats; both positional).  ``outputs``:
        ``d_kind``, ``d_index``, ``d_dist2``, ``d_point`` (the nearest points), ``d_bary``, ``d_tests`` -
        device pointers as ints to packed arrays (mrt_nearest), 0 or absent: not wanted.  ``d_dist``: the
        search radius per point (n float32), 0: unbounded.  ``d_src``: (kind, input index) pairs to
        leave out.  ``out_size``: the bytes of the structure the library may read (None: all of it).
        ``stream`` as for cast_rays_device."""
        out = _native.MrtNearest()
        for key, value in outputs.items():
            if not key.startswith("d_") or key[2:] not in self.NEAREST_FIELDS:
                raise TypeError("nearest_points_device: unknown output %r" % key)
            setattr(out, key[2:], value or None)
        batch = _native.MrtPointBatch(d_point or None, d_dist or None, d_src or None, int(stride), int(n))
        size = ctypes.sizeof(out) if out_size is None else int(out_size)
        _native.check(self._lib.mrt_nearest_points_device(self._h, ctypes.byref(batch), ctypes.byref(out), size,
                                                          ctypes.c_void_p(stream or None)))

    def nearest_points(self, points, max_dist=None, src=None, fields=None):
        """nearest_points_device for torch tensors on the renderer's device: ``points`` float32 (n, >= 3),
        ``max_dist`` float32 (n,) or None (unbounded), ``src`` (n, 2) or None, with cast_rays' stream
        joining.  Returns a dict of tensors, one per name in ``fields`` (None: all of
        ``Renderer.NEAREST_FIELDS``): int32 ``kind`` / ``index`` / ``tests`` (n,), float32 ``dist2`` (n,),
        ``point`` (n, 3) and ``bary`` (n, 2), allocated and ordered on torch's current stream.  An empty
        batch returns empty tensors."""
        import torch

        device, n, points, stride, _, _ = self._ray_tensors(points, points)
        fields = self.NEAREST_FIELDS if fields is None else tuple(fields)
        if not fields or any(f not in self.NEAREST_FIELDS for f in fields):
            raise ValueError("fields: at least one of %s" % (self.NEAREST_FIELDS,))
        if max_dist is not None:
            if max_dist.device != device or max_dist.shape != (n,):
                raise ValueError("max_dist: a tensor of shape (%d,) on %s" % (n, device))
            max_dist = max_dist.to(torch.float32).contiguous()
        if src is not None:
            if src.device != device or src.shape != (n, 2):
                raise ValueError("src: a tensor of shape (%d, 2) on %s" % (n, device))
            src = src.to(torch.int32).contiguous()
        out = {}
        for name, dtype, width in _native.NEAREST_FIELDS:
            if name in fields:
                out[name] = torch.empty(n if width == 1 else (n, width), dtype=getattr(torch, dtype), device=device)
        if n == 0:
            return out
        with self._query_stream_of(device) as stream:
            self.nearest_points_device(points.data_ptr(), n, d_dist=max_dist.data_ptr() if max_dist is not None else 0,
                                       d_src=src.data_ptr() if src is not None else 0, stride=stride, stream=stream,
                                       **{"d_" + name: x.data_ptr() for name, x in out.items()})
        return out

    # -- neighbour queries ---------------------------------------------------------------
    NEIGHBOUR_FIELDS = tuple(name for name, _, _ in _native.NEIGHBOUR_FIELDS)

    def neighbours_device(self, d_point: int, n: int, k: int, /, *, d_dist: int = 0, d_src: int = 0, stride: int = 3,
                          stream: int = 0, out_size: Optional[int] = None, **outputs: int) -> None:
        """mrt_neighbours_device: the ``k`` (1 .. 16) nearest surfaces to each of ``n`` points resident in
        device memory, in order, and the number within each point's radius.  ``outputs``: ``d_count`` and
        ``d_tests`` (n int32), ``d_kind`` / ``d_index`` (n x k int32), ``d_dist2`` (n x k float32),
        ``d_point`` (n x k x 3), ``d_bary`` (n x k x 2) - device pointers as ints to packed arrays
        (mrt_neighbours), 0 or absent: not wanted.  With ``d_count`` the walk meets every surface within
        the radius (``d_dist``; 0: unbounded, every primitive); without it, it is the K-nearest search.
        Points, ``d_dist``, ``d_src``, ``stride``, ``out_size`` and ``stream`` as for nearest_points_device."""
        out = _native.MrtNeighbours()
        for key, value in outputs.items():
            if not key.startswith("d_") or key[2:] not in self.NEIGHBOUR_FIELDS:
                raise TypeError("neighbours_device: unknown output %r" % key)
            setattr(out, key[2:], value or None)
        batch = _native.MrtPointBatch(d_point or None, d_dist or None, d_src or None, int(stride), int(n))
        size = ctypes.sizeof(out) if out_size is None else int(out_size)
        _native.check(self._lib.mrt_neighbours_device(self._h, ctypes.byref(batch), int(k), ctypes.byref(out), size,
                                                      ctypes.c_void_p(stream or None)))

    def neighbours(self, points, k: int, max_dist=None, src=None, fields=None):
        """neighbours_device for torch tensors on the renderer's device, with nearest_points' handling of
        ``points`` / ``max_dist`` / ``src`` and its stream joining.  Returns a dict of tensors, one per
        name in ``fields`` (None: all of ``Renderer.NEIGHBOUR_FIELDS``): int32 ``count`` / ``tests`` (n,),
        int32 ``kind`` / ``index`` (n, k), float32 ``dist2`` (n, k), ``point`` (n, k, 3) and ``bary``
        (n, k, 2), allocated and ordered on torch's current stream.  Leaving ``count`` out of ``fields``
        makes the walk the K-nearest search.  An empty batch returns empty tensors."""
        import torch

        device, n, points, stride, _, _ = self._ray_tensors(points, points)
        k = int(k)
        if not 1 <= k <= _native.NEIGHBOURS_MAX:
            raise ValueError("k: 1 .. %d" % _native.NEIGHBOURS_MAX)
        fields = self.NEIGHBOUR_FIELDS if fields is None else tuple(fields)
        if not fields or any(f not in self.NEIGHBOUR_FIELDS for f in fields):
            raise ValueError("fields: at least one of %s" % (self.NEIGHBOUR_FIELDS,))
        if max_dist is not None:
            if max_dist.device != device or max_dist.shape != (n,):
                raise ValueError("max_dist: a tensor of shape (%d,) on %s" % (n, device))
            max_dist = max_dist.to(torch.float32).contiguous()
        if src is not None:
            if src.device != device or src.shape != (n, 2):
                raise ValueError("src: a tensor of shape (%d, 2) on %s" % (n, device))
            src = src.to(torch.int32).contiguous()
        out = {}
        for name, dtype, width in _native.NEIGHBOUR_FIELDS:
            if name in fields:
                shape = (n,) if width == 0 else (n, k) if width == 1 else (n, k, width)
                out[name] = torch.empty(shape, dtype=getattr(torch, dtype), device=device)
        if n == 0:
            return out
        with self._query_stream_of(device) as stream:
            self.neighbours_device(points.data_ptr(), n, k, d_dist=max_dist.data_ptr() if max_dist is not None else 0,
                                   d_src=src.data_ptr() if src is not None else 0, stride=stride, stream=stream,
                                   **{"d_" + name: x.data_ptr() for name, x in out.items()})
        return out

    # -- overlap queries -----------------------------------------------------------------
    OVERLAP_FIELDS = tuple(name for name, _, _ in _native.OVERLAP_FIELDS)

    def overlap_boxes_device(self, d_mn: int, d_mx: int, n: int, k: int, /, *, mn_stride: int = 3, mx_stride: int = 3,
                             stream: int = 0, out_size: Optional[int] = None, **fields: int) -> None:
        """mrt_overlap_boxes_device: the surfaces touching each of ``n`` axis-aligned boxes resident in device
        memory (box i's min xyz at ``d_mn`` + i * ``mn_stride`` floats, its max at ``d_mx`` + i *
        ``mx_stride``), the first ``k`` (1 .. 16) by kind and input index, and their number.  ``fields``:
        ``d_any``, ``d_count``, ``d_tests`` (n int32), ``d_kind`` / ``d_index`` (n x k int32) - device
        pointers as ints to packed arrays (mrt_overlaps), 0 or absent: not wanted.  With ``d_any`` alone
        (``d_tests`` aside) the walk stops at a box's first acceptance.  ``out_size`` and ``stream`` as for
        neighbours_device."""
        out = _native.MrtOverlaps()
        for key, value in fields.items():
            if not key.startswith("d_") or key[2:] not in self.OVERLAP_FIELDS:
                raise TypeError("overlap_boxes_device: unknown output %r" % key)
            setattr(out, key[2:], value or None)
        batch = _native.MrtBoxBatch(d_mn or None, d_mx or None, int(mn_stride), int(mx_stride), int(n))
        size = ctypes.sizeof(out) if out_size is None else int(out_size)
        _native.check(self._lib.mrt_overlap_boxes_device(self._h, ctypes.byref(batch), int(k), ctypes.byref(out), size,
                                                         ctypes.c_void_p(stream or None)))

    def overlap_boxes(self, mn, mx, k: int, fields=None):
        """overlap_boxes_device for torch tensors on the renderer's device: ``mn`` / ``mx`` float32 (n, >= 3)
        (two column slices of one (n, 6) tensor are read in place), with cast_rays' stream joining.  Returns
        a dict of tensors, one per name in ``fields`` (None: all of ``Renderer.OVERLAP_FIELDS``): int32
        ``any`` / ``count`` / ``tests`` (n,) and ``kind`` / ``index`` (n, k), allocated and ordered on torch's
        current stream.  ``fields=("any",)`` is the occupancy test.  An empty batch returns empty tensors."""
        import torch

        device, n, mn, mn_stride, mx, mx_stride = self._ray_tensors(mn, mx)
        k = int(k)
        if not 1 <= k <= _native.OVERLAP_MAX:
            raise ValueError("k: 1 .. %d" % _native.OVERLAP_MAX)
        fields = self.OVERLAP_FIELDS if fields is None else tuple(fields)
        if not fields or any(f not in self.OVERLAP_FIELDS for f in fields):
            raise ValueError("fields: at least one of %s" % (self.OVERLAP_FIELDS,))
        out = {}
        for name, dtype, width in _native.OVERLAP_FIELDS:
            if name in fields:
                out[name] = torch.empty((n,) if width == 0 else (n, k), dtype=getattr(torch, dtype), device=device)
        if n == 0:
            return out
        with self._query_stream_of(device) as stream:
            self.overlap_boxes_device(mn.data_ptr(), mx.data_ptr(), n, k, mn_stride=mn_stride, mx_stride=mx_stride,
                                      stream=stream, **{"d_" + name: x.data_ptr() for name, x in out.items()})
        return out

    def voxel_occupancy(self, origin, cell, dims, field: str = "any"):
        """One overlap query (k = 1, the one ``field``: "any", "count" or "tests") over the cells of a lattice:
        ``dims`` = (nx, ny, nz) cells of size ``cell`` (a number or three) from ``origin``.  Cell (ix, iy, iz)
        has mn = origin + cell * (ix, iy, iz) and mx = origin + cell * (ix + 1, iy + 1, iz + 1) in float32, one
        multiplication and one addition, so neighbouring cells share their faces bit for bit and a triangle
        lying in a shared face is in both cells.  Returns an int32 (nz, ny, nx) tensor on the renderer's GPU."""
        import torch

        if field not in ("any", "count", "tests"):
            raise ValueError('field: "any", "count" or "tests"')
        nx, ny, nz = (int(d) for d in dims)
        if min(nx, ny, nz) < 1:
            raise ValueError("dims: three positive cell counts")
        device = torch.device("cuda", self.config.device if self.config.device >= 0 and not self.config.devices
                              else torch.cuda.current_device())
        o = torch.tensor([float(x) for x in origin], dtype=torch.float32, device=device)
        c = torch.tensor([float(x) for x in (cell if hasattr(cell, "__len__") else (cell,) * 3)], dtype=torch.float32,
                         device=device)
        iz, iy, ix = torch.meshgrid(torch.arange(nz, device=device), torch.arange(ny, device=device),
                                    torch.arange(nx, device=device), indexing="ij")
        idx = torch.stack((ix, iy, iz), dim=-1).reshape(-1, 3).to(torch.float32)
        mn = o + c * idx
        mx = o + c * (idx + 1.0)
        return self.overlap_boxes(mn, mx, 1, fields=(field,))[field].reshape(nz, ny, nx)

    # -- triangle overlap queries --------------------------------------------------------
    def overlap_triangles_device(self, d_a: int, d_b: int, d_c: int, n: int, k: int, /, *, a_stride: int = 3,
                                 b_stride: int = 3, c_stride: int = 3, stream: int = 0,
                                 out_size: Optional[int] = None, **fields: int) -> None:
        """mrt_overlap_triangles_device: the surfaces each of ``n`` query triangles resident in device memory
        touches (triangle i's corners at ``d_a`` + i * ``a_stride`` floats, ``d_b`` + i * ``b_stride``,
        ``d_c`` + i * ``c_stride``; strides of 9 with d_b = d_a + 12 bytes and d_c = d_a + 24 read an (n, 9)
        array), the first ``k`` (1 .. 16) by kind and input index, and their number.  A triangle whose corners
        coincide is a segment or a point.  ``fields``, ``out_size`` and ``stream`` as for
        overlap_boxes_device."""
        out = _native.MrtOverlaps()
        for key, value in fields.items():
            if not key.startswith("d_") or key[2:] not in self.OVERLAP_FIELDS:
                raise TypeError("overlap_triangles_device: unknown output %r" % key)
            setattr(out, key[2:], value or None)
        batch = _native.MrtTriangleBatch(d_a or None, d_b or None, d_c or None, int(a_stride), int(b_stride),
                                         int(c_stride), int(n))
        size = ctypes.sizeof(out) if out_size is None else int(out_size)
        _native.check(self._lib.mrt_overlap_triangles_device(self._h, ctypes.byref(batch), int(k), ctypes.byref(out),
                                                             size, ctypes.c_void_p(stream or None)))

    def overlap_triangles(self, tri, k: int, fields=None):
        """overlap_triangles_device for a torch float32 tensor on the renderer's device: ``tri`` (n, 9) or
        (n, 3, 3), the corners a, b, c of each query triangle, read in place (a contiguous tensor is not
        copied), with cast_rays' stream joining.  Returns a dict of tensors as overlap_boxes does.  An empty
        batch returns empty tensors."""
        import torch

        if not hasattr(tri, "dim") or tri.dtype != torch.float32 or not (
                (tri.dim() == 2 and tri.shape[1] == 9) or (tri.dim() == 3 and tuple(tri.shape[1:]) == (3, 3))):
            raise ValueError("tri: a float32 tensor of shape (n, 9) or (n, 3, 3)")
        n = tri.shape[0]
        rows = tri.reshape(n, 9)
        if rows.stride(1) != 1 or (n > 1 and rows.stride(0) < 9):
            rows = rows.contiguous()
        stride = rows.stride(0) if n > 1 else 9
        device, n, a, _, b, _ = self._ray_tensors(rows[:, 0:3], rows[:, 3:6])
        k = int(k)
        if not 1 <= k <= _native.OVERLAP_MAX:
            raise ValueError("k: 1 .. %d" % _native.OVERLAP_MAX)
        fields = self.OVERLAP_FIELDS if fields is None else tuple(fields)
        if not fields or any(f not in self.OVERLAP_FIELDS for f in fields):
            raise ValueError("fields: at least one of %s" % (self.OVERLAP_FIELDS,))
        out = {}
        for name, dtype, width in _native.OVERLAP_FIELDS:
            if name in fields:
                out[name] = torch.empty((n,) if width == 0 else (n, k), dtype=getattr(torch, dtype), device=device)
        if n == 0:
            return out
        with self._query_stream_of(device) as stream:
            base = rows.data_ptr()
            self.overlap_triangles_device(base, base + 12, base + 24, n, k, a_stride=stride, b_stride=stride,
                                          c_stride=stride, stream=stream,
                                          **{"d_" + name: x.data_ptr() for name, x in out.items()})
        return out

    def overlap_mesh(self, vertices, faces, k: int, fields=None, transform=None):
        """overlap_triangles for the triangles of a mesh: ``vertices`` float32 (v, 3) and ``faces`` integer
        (n, 3) tensors on the renderer's device; query triangle i has the corners ``vertices[faces[i]]``.
        With a 4 x 4 ``transform`` (a tensor, or anything torch.as_tensor takes) the vertices are first moved:
        ``vertices @ R.T + t`` in torch float32, R the upper-left 3 x 3 and t the last column.  The transformed
        corners' bits are torch's (its matrix product's order of operations, not this library's), and the
        answer is defined on the corners the query is given: it is overlap_triangles of exactly those floats."""
        import torch

        if not hasattr(vertices, "dim") or vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3:
            raise ValueError("vertices: a float32 tensor of shape (v, 3)")
        if not hasattr(faces, "dim") or faces.dim() != 2 or faces.shape[1] != 3 or faces.is_floating_point():
            raise ValueError("faces: an integer tensor of shape (n, 3)")
        if transform is not None:
            t = torch.as_tensor(transform, dtype=torch.float32).to(vertices.device)
            if tuple(t.shape) != (4, 4):
                raise ValueError("transform: 4 x 4")
            vertices = vertices @ t[:3, :3].T + t[:3, 3]
        tri = vertices[faces.to(device=vertices.device, dtype=torch.long)].reshape(-1, 9)
        return self.overlap_triangles(tri, k, fields=fields)

    # -- sweep queries -------------------------------------------------------------------
    SWEEP_FIELDS = tuple(name for name, _, _ in _native.SWEEP_FIELDS)

    def sweep_spheres_device(self, d_orig: int, d_dir: int, d_radius: int, n: int, /, *, d_dist: int = 0, d_src: int = 0,
                             orig_stride: int = 3, dir_stride: int = 3, stream: int = 0,
                             out_size: Optional[int] = None, **outputs: int) -> None:
        """mrt_sweep_spheres_device: the first contact of a sphere moving along each of ``n`` rays resident in
        device memory (centre ``orig`` + ``dir`` * t, ``dir`` not normalised; ``d_radius``: n float32).
        ``outputs``: ``d_hit``, ``d_kind``, ``d_index``, ``d_tests`` (n int32), ``d_t`` (n float32),
        ``d_centre`` / ``d_point`` (n x 3), ``d_bary`` (n x 2) - device pointers as ints to packed arrays
        (mrt_sweeps), 0 or absent: not wanted.  With ``d_hit`` alone (``d_tests`` aside) the walk stops at a
        ray's first acceptance.  ``d_dist``: the bound on t per ray (n float32), 0: unbounded.  ``d_src``,
        strides, ``out_size`` and ``stream`` as for nearest_points_device and cast_rays_device."""
        out = _native.MrtSweeps()
        for key, value in outputs.items():
            if not key.startswith("d_") or key[2:] not in self.SWEEP_FIELDS:
                raise TypeError("sweep_spheres_device: unknown output %r" % key)
            setattr(out, key[2:], value or None)
        batch = _native.MrtRayBatch(d_orig or None, d_dir or None, d_dist or None, d_src or None, int(orig_stride),
                                    int(dir_stride), int(n))
        size = ctypes.sizeof(out) if out_size is None else int(out_size)
        _native.check(self._lib.mrt_sweep_spheres_device(self._h, ctypes.byref(batch), ctypes.c_void_p(d_radius or None),
                                                         ctypes.byref(out), size, ctypes.c_void_p(stream or None)))

    def sweep_spheres(self, orig, dirs, radius, max_t=None, src=None, fields=None):
        """sweep_spheres_device for torch tensors on the renderer's device, with cast_rays' handling of
        ``orig`` / ``dirs`` / ``src`` and its stream joining; ``radius`` float32 (n,), ``max_t`` float32 (n,) or
        None (unbounded).  Returns a dict of tensors, one per name in ``fields`` (None: all of
        ``Renderer.SWEEP_FIELDS``): int32 ``hit`` / ``kind`` / ``index`` / ``tests`` (n,), float32 ``t`` (n,),
        ``centre`` / ``point`` (n, 3) and ``bary`` (n, 2), allocated and ordered on torch's current stream.
        ``fields=("hit",)`` is the "is this move free" test.  An empty batch returns empty tensors."""
        import torch

        device, n, orig, orig_stride, dirs, dir_stride = self._ray_tensors(orig, dirs)
        fields = self.SWEEP_FIELDS if fields is None else tuple(fields)
        if not fields or any(f not in self.SWEEP_FIELDS for f in fields):
            raise ValueError("fields: at least one of %s" % (self.SWEEP_FIELDS,))
        if radius.device != device or radius.shape != (n,):
            raise ValueError("radius: a tensor of shape (%d,) on %s" % (n, device))
        radius = radius.to(torch.float32).contiguous()
        if max_t is not None:
            if max_t.device != device or max_t.shape != (n,):
                raise ValueError("max_t: a tensor of shape (%d,) on %s" % (n, device))
            max_t = max_t.to(torch.float32).contiguous()
        if src is not None:
            if src.device != device or src.shape != (n, 2):
                raise ValueError("src: a tensor of shape (%d, 2) on %s" % (n, device))
            src = src.to(torch.int32).contiguous()
        out = {}
        for name, dtype, width in _native.SWEEP_FIELDS:
            if name in fields:
                out[name] = torch.empty(n if width == 1 else (n, width), dtype=getattr(torch, dtype), device=device)
        if n == 0:
            return out
        with self._query_stream_of(device) as stream:
            self.sweep_spheres_device(orig.data_ptr(), dirs.data_ptr(), radius.data_ptr(), n,
                                      d_dist=max_t.data_ptr() if max_t is not None else 0,
                                      d_src=src.data_ptr() if src is not None else 0, orig_stride=orig_stride,
                                      dir_stride=dir_stride, stream=stream,
                                      **{"d_" + name: x.data_ptr() for name, x in out.items()})
        return out

    def first_hit_planes(self, camera=None, sample: int = 0, fields=None):
        """The first hit of every pixel's camera ray (sample ``sample``) as planes: camera_rays(camera,
        sample_base=sample, spp=1), then cast_hits, scattered by ``pixels`` into (height, width) or
        (height, width, c) tensors - the guide planes (albedo ``kd``, ``normal``, depth ``t``) a
        denoiser wants for a frame.  Pixels this shard does not own keep ``kind`` 0, ``index`` and
        ``material`` -1, ``texCoord`` -1 and 0 elsewhere."""
        import torch

        orig, dirs, _, pixels = self.camera_rays(camera, sample_base=sample, spp=1)
        recs = self.cast_hits(orig, dirs, fields=fields)
        h, w = self.config.height, self.config.width
        at = pixels.to(torch.int64)
        planes = {}
        for name, x in recs.items():
            fill = -1 if name in ("index", "material", "texCoord") else 0
            plane = torch.full((h * w,) + tuple(x.shape[1:]), fill, dtype=x.dtype, device=x.device)
            plane[at] = x
            planes[name] = plane.reshape((h, w) + tuple(x.shape[1:]))
        return planes

    # -- shaded ray queries --------------------------------------------------------------
    def shade_rays_device(self, d_orig: int, d_dir: int, n: int, *, d_key: int = 0, d_src: int = 0,
                          orig_stride: int = 3, dir_stride: int = 3, d_rgb: int, rgb_stride: int = 3,
                          stream: int = 0):
        """mrt_shade_rays_device: the radiance arriving along ``n`` rays resident in device memory -
        the renderer's whole ray tree (shader, maxDepth, samplesLight) under each ray, taken as the
        depth-1 ray of a path with key ``d_key[i]`` (0: ``path_key(i, 0)``) - as linear float RGB at
        ``d_rgb + i * rgb_stride``.  Pointers as ints, strides in floats; ``d_src`` as for
        cast_rays_device.  Ordered after ``stream``'s earlier work; returns, with the radiance
        written, the (rays, shadow rays) the batch built.  Frames do not see the call."""
        batch = _native.MrtShadeBatch(
            _native.MrtRayBatch(d_orig or None, d_dir or None, None, d_src or None, int(orig_stride), int(dir_stride),
                                int(n)), d_key or None)
        rays = (ctypes.c_uint64 * 2)()
        _native.check(self._lib.mrt_shade_rays_device(
            self._h, ctypes.byref(batch), ctypes.c_void_p(d_rgb or None), int(rgb_stride), rays,
            ctypes.c_void_p(stream or None)))
        return int(rays[0]), int(rays[1])

    def shade_rays(self, orig, dirs, keys=None, src=None):
        """shade_rays_device for torch tensors on the renderer's device, with cast_rays' handling of
        ``orig`` / ``dirs`` / ``src``; ``keys``: (n,) path keys (any integer dtype holding their 32 bits;
        None: ``path_key(i, 0)``).  Returns the radiance, float32 (n, 3), allocated and ordered on
        torch's current stream; an empty batch returns an empty tensor."""
        import torch

        device, n, orig, orig_stride, dirs, dir_stride = self._ray_tensors(orig, dirs)
        if keys is not None:
            if keys.device != device or keys.shape != (n,) or keys.dtype.is_floating_point:
                raise ValueError("keys: an integer tensor of shape (%d,) on %s" % (n, device))
            # the keys' 32 bits as int32 (few torch kernels take uint32; a wider dtype wraps)
            if keys.dtype == torch.uint32:
                keys = keys.contiguous().view(torch.int32)
            elif keys.dtype != torch.int32:
                keys = keys.to(torch.int64).to(torch.int32)
            keys = keys.contiguous()
        if src is not None:
            if src.device != device or src.shape != (n, 2):
                raise ValueError("src: a tensor of shape (%d, 2) on %s" % (n, device))
            src = src.to(torch.int32).contiguous()
        rgb = torch.empty((n, 3), dtype=torch.float32, device=device)
        if n == 0:
            return rgb
        with self._query_stream_of(device) as stream:
            self.shade_rays_device(orig.data_ptr(), dirs.data_ptr(), n, d_key=keys.data_ptr() if keys is not None else 0,
                                   d_src=src.data_ptr() if src is not None else 0, orig_stride=orig_stride,
                                   dir_stride=dir_stride, d_rgb=rgb.data_ptr(), stream=stream)
        return rgb

    def camera_rays(self, camera=None, sample_base: int = 0, spp: Optional[int] = None):
        """mrt_camera_rays_device: the renderer's camera rays as a batch for shade_rays / cast_rays -
        (orig (n, 3), dirs (n, 3) float32, keys (n,) uint32, pixels (n,) int32) torch tensors on the
        renderer's GPU, path ``slot * spp + s`` in this shard's slot order, samples ``sample_base ..
        sample_base + spp - 1`` (``spp`` None: samplesPixel).  ``camera``: set_camera's tuple for
        another view through the renderer's pixel sampler; None: the renderer's camera."""
        import torch

        spp = int(spp) if spp else max(1, self.config.samplesPixel)
        n = self.scene_info()["pixelSlots"] * spp
        device = torch.device("cuda", self.config.device if self.config.device >= 0 and not self.config.devices
                              else torch.cuda.current_device())
        orig = torch.empty((n, 3), dtype=torch.float32, device=device)
        dirs = torch.empty((n, 3), dtype=torch.float32, device=device)
        keys = torch.empty(n, dtype=torch.int32, device=device).view(torch.uint32)
        pixels = torch.empty(n, dtype=torch.int32, device=device)
        if n == 0:
            return orig, dirs, keys, pixels
        view = self._views([camera]) if camera is not None else None
        # (ordered on torch's current stream as the other queries are: handle 0 would be the renderer's
        # own stream, and a reader on torch's null stream could then see the tensors before the kernel ran)
        with self._query_stream_of(device) as stream:
            got = self._lib.mrt_camera_rays_device(self._h, view, int(sample_base), spp, orig.data_ptr(), dirs.data_ptr(),
                                                   keys.data_ptr(), pixels.data_ptr(), ctypes.c_void_p(stream or None))
        if got != n:
            _native.check(-1 if got < 0 else 0)
            raise RuntimeError("mrt_camera_rays_device returned %d paths, %d expected" % (got, n))
        return orig, dirs, keys, pixels

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.mrt_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def walk_tree(config: Config):
    """Host-side quantized wide walk tree of the configured scene (no GPU): nodes (N, 4W) uint32
    (3W box words, W child references), grid (6,) float32 (origin xyz, step xyz), root (3,) int32
    (reference, triangle count, width W) - DESIGN.md section 3.1."""
    lib = _native.lib()
    c = config.to_c()
    n = lib.mrt_walk_tree(ctypes.byref(c), None, None, None)
    if n < 0:
        raise RuntimeError(lib.mrt_last_error().decode())
    # the width first (a node is 4 * width words), then the nodes
    grid = np.empty(6, np.float32)
    root = np.empty(3, np.int32)
    lib.mrt_walk_tree(ctypes.byref(c), None, _ptr(grid), _ptr(root))
    nodes = np.empty((n, 4 * int(root[2])), np.uint32)
    if lib.mrt_walk_tree(ctypes.byref(c), _ptr(nodes), _ptr(grid), _ptr(root)) != n:
        raise RuntimeError(lib.mrt_last_error().decode())
    return nodes, grid, root


def walk_stack(config: Config) -> dict:
    """Host only (mrt_walk_stack): what the configured scene's trees ask of the walks' stacks, as the
    renderer works it out at load.  ``need``: stack entries (``Renderer.get_tuning(40)``; the packet
    walk serves up to 128), ``quantized``: False where a box or the grid is not finite and every ray
    walks the reference tree, ``refDepth`` / ``walkDepth`` / ``wideDepth``: levels of the reference
    tree, the binary walk tree and the wide walk tree, ``spillDepth``: entries of a thread's spill area."""
    out = np.zeros(6, np.int32)
    c = config.to_c()
    _native.check(_native.lib().mrt_walk_stack(ctypes.byref(c), _ptr(out)))
    return {"need": int(out[0]), "quantized": bool(out[1]), "refDepth": int(out[2]), "walkDepth": int(out[3]),
            "wideDepth": int(out[4]), "spillDepth": int(out[5])}


def plan_spill(threads: int, stack_need: int, avail_bytes: int = 0) -> int:
    """Host only (mrt_plan_spill): the bytes of the walks' two spill areas for ``threads`` resident
    walk threads and a stack need.  Raises RuntimeError where a renderer refuses the scene at load:
    the areas' 32-bit offsets would pass 2^31, or they exceed ``avail_bytes`` (0: not checked)."""
    n = _native.lib().mrt_plan_spill(int(threads), int(stack_need), int(avail_bytes))
    if n < 0:
        raise RuntimeError(_native.lib().mrt_last_error().decode())
    return int(n)


def triangle_bvh(config: Config):
    """Host-side triangle BVH of the configured scene (no GPU): boxes (N, 6), offsets, counts,
    order - the layout of the reference's BVHNode array (BVH.hpp:56-60)."""
    lib = _native.lib()
    c = config.to_c()
    n = lib.mrt_triangle_bvh(ctypes.byref(c), None, None, None, None)
    if n < 0:
        raise RuntimeError(lib.mrt_last_error().decode())
    boxes = np.empty((n, 6), np.float32)
    off, cnt = np.empty(n, np.int32), np.empty(n, np.int32)
    order = np.full((n + 1) // 2, -1, np.int32)  # 2 * triangles - 1 slots (a lone root: 0 or 1 triangle)
    n2 = lib.mrt_triangle_bvh(ctypes.byref(c), _ptr(boxes), _ptr(off), _ptr(cnt), _ptr(order))
    if n2 != n:
        raise RuntimeError(lib.mrt_last_error().decode())
    return boxes, off, cnt, order[:int(cnt[0])] if n == 1 else order


def _scene_arrays(name, config, shapes):
    """A host-only scene accessor (mrt_scene_*): the count first, then the arrays of the given
    (dtype, per-item shape) filled in the scene's input order."""
    lib = _native.lib()
    fn = getattr(lib, name)
    c = config.to_c()
    n = fn(ctypes.byref(c), *([None] * len(shapes)))
    if n < 0:
        raise RuntimeError(lib.mrt_last_error().decode())
    arrays = [np.zeros((n,) + shape, dtype) for dtype, shape in shapes]
    if fn(ctypes.byref(c), *[_ptr(a) for a in arrays]) != n:
        raise RuntimeError(lib.mrt_last_error().decode())
    return arrays


def scene_triangles(config: Config):
    """Host only (mrt_scene_triangles): the configured scene's triangles in input order - the order
    ``index`` of the ray queries refers to - as the renderer holds them: geom (T, 3, 3) float32 (A, AB,
    AC), normals (T, 3, 3) (nA, nB, nC), texCoords (T, 3, 2) (-1 where none), material (T,) int32."""
    return tuple(_scene_arrays("mrt_scene_triangles", config, [(np.float32, (3, 3)), (np.float32, (3, 3)),
                                                               (np.float32, (3, 2)), (np.int32, ())]))


def scene_planes(config: Config):
    """Host only (mrt_scene_planes): normalPoint (P, 2, 3) float32 (normal, point), material (P,) int32."""
    return tuple(_scene_arrays("mrt_scene_planes", config, [(np.float32, (2, 3)), (np.int32, ())]))


def scene_spheres(config: Config):
    """Host only (mrt_scene_spheres): centreSqRadius (S, 4) float32, material (S,) int32."""
    return tuple(_scene_arrays("mrt_scene_spheres", config, [(np.float32, (4,)), (np.int32, ())]))


def scene_materials(config: Config):
    """Host only (mrt_scene_materials): coeffs (M, 13) float32 (Le, Kd, Ks, Kt, ior) in the order
    ``material`` of cast_hits refers to, texture (M,) int32 (the texture id, -1: none)."""
    return tuple(_scene_arrays("mrt_scene_materials", config, [(np.float32, (13,)), (np.int32, ())]))


def scene_lights(config: Config):
    """Host only (mrt_scene_lights): kind (L,) int32 (0 point, 1 area), geom (L, 3, 3) float32 (A, AB, AC
    of an area light; a point light's position, then zeros), coeffs (L, 13) float32: the light's own
    material, which a light hit of cast_hits names as ``material`` = M + the light's index."""
    return tuple(_scene_arrays("mrt_scene_lights", config, [(np.int32, ()), (np.float32, (3, 3)), (np.float32, (13,))]))


def plan_queues(levels: int, branching: int, pixel_slots: int, samples_pixel: int = 1, samples_light: int = 1,
                textured: bool = False, path_budget: int = 0, byte_budget: int = 0, growth_pct: int = 0,
                slack: int = -1, worst_case: bool = False, demand: Optional[dict] = None,
                previous: Optional[dict] = None) -> dict:
    """The renderer's queue planner (mrt_plan_queues, host only; DESIGN.md section 2, "Queue plans").

    Without ``demand``: the first allocation.  ``demand`` is the record of an overflowed pass:
    ``{"mask": bit l = depth l's queue dropped a write, "chunkSlots", "paths": level-1 paths of
    that chunk, "seg": per depth the largest segment's requested rays, "shadowSeg": ... shadow
    rays}``.  ``previous`` is the plan that pass ran with (a dict as returned here): no capacity
    per path shrinks.  ``worst_case``: every level holds all the rays a chunk can spawn.
    Returns ``{"chunkSlots", "segCap", "shadowSegCap", "bytes", "worstCase"}`` (the lists: one
    entry per level, slots per queue segment; a queue is 8 segments).  Raises RuntimeError when no
    chunk fits the byte budget."""
    q = _native.MrtQueuePlanRequest()
    q.levels, q.branching, q.samplesPixel, q.samplesLight = levels, branching, samples_pixel, samples_light
    q.textured, q.segments, q.growthPct, q.slack = int(textured), 0, growth_pct, slack
    q.worstCase, q.pixelSlots, q.pathBudget, q.byteBudget = int(worst_case), pixel_slots, path_budget, byte_budget
    if demand is not None:
        q.hasDemand = 1
        q.overflowMask = int(demand["mask"])
        q.demandChunkSlots = int(demand["chunkSlots"])
        q.demandPaths = int(demand["paths"])
        for i, v in enumerate(demand["seg"]):
            q.segDemand[i] = int(v)
        for i, v in enumerate(demand["shadowSeg"]):
            q.shadowSegDemand[i] = int(v)
    if previous is not None:
        q.prevChunkSlots = int(previous["chunkSlots"])
        for i, v in enumerate(previous["segCap"]):
            q.prevSegCap[i] = int(v)
        for i, v in enumerate(previous["shadowSegCap"]):
            q.prevShadowSegCap[i] = int(v)
    plan = _native.MrtQueuePlan()
    _native.check(_native.lib().mrt_plan_queues(ctypes.byref(q), ctypes.byref(plan)))
    return {"chunkSlots": int(plan.chunkSlots), "segCap": list(plan.segCap)[:levels],
            "shadowSegCap": list(plan.shadowSegCap)[:levels], "bytes": int(plan.bytes),
            "worstCase": bool(plan.worstCase)}


def regular_grid(config: Config, kind: int):
    """Host-side RegularGrid (accelerator 2, RegularGrid.hpp with gridSize 32) of one primitive
    kind of the configured scene (0 planes, 1 spheres, 2 triangles), no GPU: world (12 floats:
    min, max, cellSize, cellSizeInverted), start (32^3 + 1), items (input indices)."""
    lib = _native.lib()
    c = config.to_c()
    n = lib.mrt_regular_grid(ctypes.byref(c), kind, None, None, None)
    if n < 0:
        raise RuntimeError(lib.mrt_last_error().decode())
    world, start, items = np.empty(12, np.float32), np.empty(32 ** 3 + 1, np.int32), np.empty(max(n, 1), np.int32)
    if lib.mrt_regular_grid(ctypes.byref(c), kind, _ptr(world), _ptr(start), _ptr(items)) != n:
        raise RuntimeError(lib.mrt_last_error().decode())
    return world, start, items[:n]


def grid_box_test(kind: int, prim, box) -> bool:
    """The RegularGrid fill's cell membership test (Triangle / Plane / Sphere::intersect(const
    AABB&)) as the renderer's host build evaluates it.  kind 0 prim = A + B + C, 1 = point +
    normal, 2 = center + (radius,); box = min + max."""
    p = np.ascontiguousarray(prim, np.float32)
    b = np.ascontiguousarray(box, np.float32)
    rc = _native.lib().mrt_grid_box_test(kind, _ptr(p), _ptr(b))
    if rc < 0:
        raise ValueError(_native.lib().mrt_last_error().decode())
    return bool(rc)


def decode_texture(path: str) -> np.ndarray:
    """A map_Kd texture decoded as the renderer loads it (Texture::createTexture,
    Texture.cpp:83-114): (height, width, channels) uint8.  Host only."""
    lib = _native.lib()
    dims = np.zeros(3, np.int32)
    n = lib.mrt_decode_texture(path.encode(), _ptr(dims), None)
    if n < 0:
        raise RuntimeError(lib.mrt_last_error().decode())
    out = np.empty(int(n), np.uint8)
    lib.mrt_decode_texture(path.encode(), _ptr(dims), _ptr(out))
    return out.reshape(int(dims[1]), int(dims[0]), int(dims[2]))


def sample_tables():
    """Host only: (shader table, sampler table, trig (2^20 x cos, sin)) as the renderer builds them."""
    a, b, t = np.empty(1 << 20, np.float32), np.empty(1 << 20, np.float32), np.empty(2 << 20, np.float32)
    _native.check(_native.lib().mrt_sample_tables(_ptr(a), _ptr(b), _ptr(t)))
    return a, b, t.reshape(-1, 2)


def kat_slab(boxes, orig, dirs):
    """The device slab test (AABB.cpp:34-54) on (box, ray) pairs: (reference predicate,
    IEEE-min/max form, 1/d finite) per pair, int32 (n, 3)."""
    b = np.ascontiguousarray(boxes, np.float32)
    o = np.ascontiguousarray(orig, np.float32)
    d = np.ascontiguousarray(dirs, np.float32)
    out = np.empty((len(b), 3), np.int32)
    _native.check(_native.lib().mrt_kat_slab(_ptr(b), _ptr(o), _ptr(d), len(b), _ptr(out)))
    return out


def kat_triangle(tris, orig, dirs):
    """The device triangle test (Triangle.cpp:63-109) on (triangle A B C, ray) pairs: hit, t."""
    tr = np.ascontiguousarray(tris, np.float32)
    o = np.ascontiguousarray(orig, np.float32)
    d = np.ascontiguousarray(dirs, np.float32)
    hit, t = np.empty(len(tr), np.int32), np.empty(len(tr), np.float32)
    _native.check(_native.lib().mrt_kat_triangle(_ptr(tr), _ptr(o), _ptr(d), len(tr), _ptr(hit), _ptr(t)))
    return hit, t


def _point_distance(fn, kind, prims, points):
    kind = int(kind)
    width = {1: 6, 2: 4, 3: 9, 4: 9}.get(kind, 9)
    pr = np.ascontiguousarray(prims, np.float32).reshape(-1, width)
    pt = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    if len(pr) != len(pt):
        raise ValueError("point_distance: as many primitives as points")
    d2 = np.empty(len(pt), np.float32)
    q, uv = np.empty((len(pt), 3), np.float32), np.empty((len(pt), 2), np.float32)
    _native.check(fn(kind, _ptr(pr), _ptr(pt), len(pt), _ptr(d2), _ptr(q), _ptr(uv)))
    return d2, q, uv


def point_distance(kind, prims, points):
    """mrt_point_distance (host, no GPU): the nearest-point query's distance functions on (primitive,
    point) pairs.  kind 1: plane (normal, point); 2: sphere (centre, sqRadius); 3 / 4: triangle / area
    light (A, AB, AC).  Returns dist2 (n,), nearest (n, 3), bary (n, 2), float32."""
    return _point_distance(_native.lib().mrt_point_distance, kind, prims, points)


def kat_point_distance(kind, prims, points):
    """The same pairs through the device's distance functions (needs a GPU)."""
    return _point_distance(_native.lib().mrt_kat_point_distance, kind, prims, points)


def _box_overlap(fn, kind, prims, boxes):
    kind = int(kind)
    width = {1: 6, 2: 4, 3: 9, 4: 9}.get(kind, 9)
    pr = np.ascontiguousarray(prims, np.float32).reshape(-1, width)
    bx = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
    if len(pr) != len(bx):
        raise ValueError("box_overlap: as many primitives as boxes")
    out = np.empty(len(bx), np.int32)
    _native.check(fn(kind, _ptr(pr), _ptr(bx), len(bx), _ptr(out)))
    return out


def box_overlap(kind, prims, boxes):
    """mrt_box_overlap (host, no GPU): the overlap query's functions on (primitive, box) pairs.  kind and
    prims as for point_distance; boxes (n, 6): min xyz, max xyz.  Returns int32 (n,): 1 accepted, 0 not."""
    return _box_overlap(_native.lib().mrt_box_overlap, kind, prims, boxes)


def kat_box_overlap(kind, prims, boxes):
    """The same pairs through the device's overlap functions (needs a GPU)."""
    return _box_overlap(_native.lib().mrt_kat_box_overlap, kind, prims, boxes)


def _triangle_overlap(fn, kind, prims, tris):
    kind = int(kind)
    width = {1: 6, 2: 4, 3: 9, 4: 9}.get(kind, 9)
    pr = np.ascontiguousarray(prims, np.float32).reshape(-1, width)
    tr = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
    if len(pr) != len(tr):
        raise ValueError("triangle_overlap: as many primitives as triangles")
    out = np.empty(len(tr), np.int32)
    _native.check(fn(kind, _ptr(pr), _ptr(tr), len(tr), _ptr(out)))
    return out


def triangle_overlap(kind, prims, tris):
    """mrt_triangle_overlap (host, no GPU): the triangle overlap query's functions on (primitive, triangle)
    pairs.  kind and prims as for point_distance; tris (n, 9) or (n, 3, 3): the corners a, b, c.  Returns int32
    (n,): 1 accepted, 0 not."""
    return _triangle_overlap(_native.lib().mrt_triangle_overlap, kind, prims, tris)


def kat_triangle_overlap(kind, prims, tris):
    """The same pairs through the device's triangle overlap functions (needs a GPU)."""
    return _triangle_overlap(_native.lib().mrt_kat_triangle_overlap, kind, prims, tris)


def _sphere_sweep(fn, kind, prims, rays):
    kind = int(kind)
    width = {1: 6, 2: 4, 3: 9, 4: 9}.get(kind, 9)
    pr = np.ascontiguousarray(prims, np.float32).reshape(-1, width)
    ry = np.ascontiguousarray(rays, np.float32).reshape(-1, 7)
    if len(pr) != len(ry):
        raise ValueError("sphere_sweep: as many primitives as sweeps")
    n = len(ry)
    hit, t = np.empty(n, np.int32), np.empty(n, np.float32)
    centre, point, bary = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32), np.empty((n, 2), np.float32)
    _native.check(fn(kind, _ptr(pr), _ptr(ry), n, _ptr(hit), _ptr(t), _ptr(centre), _ptr(point), _ptr(bary)))
    return hit, t, centre, point, bary


def sphere_sweep(kind, prims, rays):
    """mrt_sphere_sweep (host, no GPU): the sweep query's functions on (primitive, sweep) pairs.  kind and
    prims as for point_distance; rays (n, 7): o xyz, d xyz, r.  Returns (hit int32 (n,), t float32 (n,) - +inf on
    a miss, centre (n, 3), point (n, 3), bary (n, 2))."""
    return _sphere_sweep(_native.lib().mrt_sphere_sweep, kind, prims, rays)


def kat_sphere_sweep(kind, prims, rays):
    """The same pairs through the device's sweep functions (needs a GPU)."""
    return _sphere_sweep(_native.lib().mrt_kat_sphere_sweep, kind, prims, rays)


def kat_accumulate(rgb, spp, sample_base, bitmap, width, height, mode=0):
    """The accumulation kernels (incrementalAvg, Utils.cpp:66-90) on given radiance: rgb (nSlots * spp, 3)
    float32, slot-major; bitmap (width * height) int32, read when sample_base > 0 and updated in
    place; slot q is sharding.slot_pixels(width, height, 0, 1)[q].  mode 0: k_accumulate, 1:
    k_resolve_accumulate (every vertex terminal).  False (bitmap untouched) where mode 1 is not
    launched (spp does not divide 64)."""
    c = np.ascontiguousarray(rgb, np.float32).reshape(-1, 3)
    assert len(c) % spp == 0
    assert bitmap.dtype == np.int32 and bitmap.size == width * height and bitmap.flags["C_CONTIGUOUS"]
    launched = ctypes.c_int32(0)
    _native.check(_native.lib().mrt_kat_accumulate(_ptr(c), len(c) // spp, spp, sample_base, width, height, mode,
                                                   _ptr(bitmap), ctypes.byref(launched)))
    return bool(launched.value)


_active: List[Renderer] = []


def ray_trace(config: Config, async_: bool = False):
    """RayTrace(Config&, bool) (C_wrapper.cpp:36-290): build, render `repeats` frames into
    config.bitmap, print the reference's summary lines."""
    def work():
        if config.bitmap is None:
            config.bitmap = np.zeros(config.width * config.height, np.int32)
        t0 = time.perf_counter()
        # progressive, as C_wrapper's render loop: the caller may read config.bitmap meanwhile
        r = Renderer(dataclasses.replace(config, progressive=1))
        t1 = time.perf_counter()
        _active.append(r)
        try:
            repeats = config.repeats
            t2 = time.perf_counter()
            while True:
                r.render_frame(config.bitmap, config.threads)
                repeats -= 1
                if repeats <= 0:
                    break
            secs = time.perf_counter() - t2
            rays = r.get_total_casted_rays()
            if config.printStdOut:
                info = r.scene_info()
                print(f"TRIANGLES = {info['triangles']}")
                print(f"LIGHTS = {info['lights']}")
                print(f"Creating Time in secs = {t1 - t0}")
                print(f"Rendering Time in secs = {secs}")
                print(f"Casted rays = {rays}")
                print(f"width = {config.width}")
                print(f"height = {config.height}")
                print(f"Total Millions rays per second = {rays / secs / 1e6}")
        finally:
            _active.remove(r)
            r.close()
    if async_:
        th = threading.Thread(target=work, daemon=True)
        th.start()
        return th
    work()
    return None


def path_key(pixel: int, sample: int) -> int:
    """mrt_path_key (host only): the key every sampler draw of the path of (pixel index y * width + x,
    sample) derives from - what shade_rays takes as ``keys``."""
    return int(_native.lib().mrt_path_key(int(pixel) & 0xFFFFFFFF, int(sample) & 0xFFFFFFFF))


def stop_render():
    """stopRender() (C_wrapper.cpp:271-275)."""
    for r in list(_active):
        r.stop_render()
