"""ORACLE — TEST INFRASTRUCTURE ONLY (ctypes wrapper of oracle/build/libmrt_oracle.so).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module.
The library is a CPU restatement of the reference render path (see mrt_oracle.cpp's header
for what pins it and where parity is unpinned).
"""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "build", "libmrt_oracle.so")


def build():
    subprocess.run(["make", "-s", "-C", HERE], check=True)


class _Cfg(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in
                ("width", "height", "shader", "sceneIndex", "samplesPixel", "samplesLight", "maxDepth")] + \
               [("obj", ctypes.c_char_p), ("mtl", ctypes.c_char_p), ("cam", ctypes.c_char_p),
                ("accelerator", ctypes.c_int32)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            build()
        L = ctypes.CDLL(LIB)
        vp, P = ctypes.c_void_p, ctypes.POINTER
        f = ctypes.POINTER(ctypes.c_float)
        L.oracle_create.restype = vp
        L.oracle_create.argtypes = [P(_Cfg)]
        L.oracle_destroy.argtypes = [vp]
        L.oracle_set_faithful.argtypes = [vp, ctypes.c_int]
        L.oracle_num_tiles.argtypes = [vp]
        L.oracle_render.restype = ctypes.c_uint64
        L.oracle_render.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.oracle_render_tiles.restype = ctypes.c_uint64
        L.oracle_render_tiles.argtypes = [vp, vp, ctypes.c_int, vp, ctypes.c_int]
        L.oracle_counts.argtypes = [vp, vp]
        L.oracle_primary_hits.argtypes = [vp, vp, vp, vp]
        L.oracle_trace_rays.argtypes = [vp, vp, vp, vp, vp, ctypes.c_int32, ctypes.c_int, vp, vp, vp]
        L.oracle_shade_rays.restype = ctypes.c_uint64
        L.oracle_shade_rays.argtypes = [vp, vp, vp, vp, vp, ctypes.c_int32, ctypes.c_int, vp]
        L.oracle_camera_rays.restype = ctypes.c_int64
        L.oracle_camera_rays.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
        L.oracle_triangle_bvh.restype = ctypes.c_int64
        L.oracle_triangle_bvh.argtypes = [vp, vp, vp, vp, vp]
        L.oracle_kat_triangle.argtypes = [f, f, f, f, f, ctypes.c_int, f]
        L.oracle_kat_aabb.argtypes = [f, f, f, f]
        L.oracle_aabb_props.argtypes = [f, f, f, f]
        L.oracle_triangle_aabb.argtypes = [f, f, f, f, f]
        L.oracle_kat_plane.argtypes = [f, f, f, f, f]
        L.oracle_plane_aabb.argtypes = [f, f, f, f]
        L.oracle_kat_sphere.argtypes = [f, ctypes.c_float, f, f, f]
        L.oracle_set_pixel_value.argtypes = [vp, ctypes.c_float]
        L.oracle_kat_camera.argtypes = [ctypes.c_char_p, ctypes.c_float, f]
        L.oracle_halton.restype = ctypes.c_float
        L.oracle_halton.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
        L.oracle_table.argtypes = [ctypes.c_uint32, vp]
        L.oracle_hemisphere_trig.argtypes = [vp]
        L.oracle_path_key.restype = ctypes.c_uint32
        L.oracle_path_key.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
        L.oracle_sample_index.restype = ctypes.c_uint32
        L.oracle_sample_index.argtypes = [ctypes.c_uint32] * 3
        L.oracle_incremental_avg.restype = ctypes.c_int32
        L.oracle_incremental_avg.argtypes = [ctypes.c_float] * 3 + [ctypes.c_int32] * 2
        L.oracle_fast_arctan.restype = ctypes.c_float
        L.oracle_fast_arctan.argtypes = [ctypes.c_float]
        L.oracle_selftest_partition.argtypes = [ctypes.c_uint32, ctypes.c_int]
        L.oracle_register_texture.argtypes = [ctypes.c_char_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, vp]
        L.oracle_grid_box_test.argtypes = [ctypes.c_int, f, f]
        L.oracle_regular_grid.restype = ctypes.c_int64
        L.oracle_regular_grid.argtypes = [vp, ctypes.c_int, vp, vp, vp]
        _lib = L
    return _lib


def decode_png(path):
    """PNG -> (height, width, channels) uint8 with stb_image's conventions (Texture.cpp:83-114:
    stbi_load_from_memory, req_comp 0): palette -> RGB (RGBA with tRNS), tRNS key adds alpha to
    grey / RGB, grey below 8 bits scaled to 0..255, 16-bit samples -> high byte.  Non-interlaced."""
    import struct
    import zlib
    data = open(path, "rb").read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("not a PNG")
    pos, idat, plte, trns, hdr = 8, b"", b"", b"", None
    while pos + 8 <= len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        pos += 12 + n
        if kind == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"PLTE":
            plte = body
        elif kind == b"tRNS":
            trns = body
        elif kind == b"IDAT":
            idat += body
        elif kind == b"IEND":
            break
    w, h, depth, ctype, _, _, interlace = hdr
    if interlace:
        raise ValueError("interlaced PNG")
    chans = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ctype]
    row = (w * chans * depth + 7) // 8
    bpp = max(1, chans * depth // 8)
    raw = zlib.decompress(idat)
    out = np.zeros((h, row), np.int32)
    prev = np.zeros(row, np.int32)
    for y in range(h):
        f = raw[y * (row + 1)]
        cur = np.frombuffer(raw, np.uint8, row, y * (row + 1) + 1).astype(np.int32)
        rec = np.zeros(row, np.int32)
        for x in range(row):
            a = rec[x - bpp] if x >= bpp else 0
            b = prev[x]
            c = prev[x - bpp] if x >= bpp else 0
            if f == 0:
                pred = 0
            elif f == 1:
                pred = a
            elif f == 2:
                pred = b
            elif f == 3:
                pred = (a + b) // 2
            else:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
            rec[x] = (cur[x] + pred) & 0xFF
        out[y] = rec
        prev = rec
    # samples
    if depth == 8:
        s = out[:, :w * chans].reshape(h, w, chans)
    elif depth == 16:
        s = (out[:, 0::2][:, :w * chans] << 8 | out[:, 1::2][:, :w * chans]).reshape(h, w, chans)
    else:
        per = 8 // depth
        bits = np.zeros((h, row * per), np.int32)
        for k in range(per):
            bits[:, k::per] = (out >> (8 - depth * (k + 1))) & ((1 << depth) - 1)
        s = bits[:, :w * chans].reshape(h, w, chans)
    if ctype == 3:
        pal = np.frombuffer(plte, np.uint8).reshape(-1, 3)
        img = pal[s[:, :, 0]]
        if trns:
            alpha = np.full(256, 255, np.uint8)
            alpha[:len(trns)] = np.frombuffer(trns, np.uint8)
            img = np.concatenate([img, alpha[s[:, :, 0]][:, :, None]], 2)
        return np.ascontiguousarray(img.astype(np.uint8))
    img = (s >> 8) if depth == 16 else (s * {1: 0xFF, 2: 0x55, 4: 0x11, 8: 1}[depth])
    if trns and ctype in (0, 2):
        key = np.array(struct.unpack(">" + "H" * chans, trns[:2 * chans]))
        alpha = np.where(np.all(s == key, axis=2), 0, 255)
        img = np.concatenate([img, alpha[:, :, None]], 2)
    return np.ascontiguousarray(img.astype(np.uint8))


def register_textures(obj, mtl):
    """Decode the map_Kd images an MTL names (beside the OBJ) and hand them to the oracle."""
    if not mtl or not os.path.exists(mtl):
        return
    base = os.path.dirname(obj)
    for line in open(mtl):
        t = line.strip().split(None, 1)
        if len(t) == 2 and t[0] == "map_Kd":
            path = os.path.join(base, t[1].strip()) if base else t[1].strip()
            if os.path.exists(path):
                img = decode_png(path)
                lib().oracle_register_texture(path.encode(), img.shape[1], img.shape[0], img.shape[2],
                                              img.ctypes.data)


def fvec(*v):
    a = (ctypes.c_float * len(v))(*[float(x) for x in v])
    return a


class Oracle:
    """CPU reference renderer for one configuration (same meaning as mobileraytracer_amd.Config)."""

    def __init__(self, width, height, shader=1, sceneIndex=0, samplesPixel=1, samplesLight=1, maxDepth=6,
                 obj="", mtl="", cam="", accelerator=3):
        self.width, self.height, self.samples_pixel = width, height, samplesPixel
        self._keep = [s.encode() for s in (obj, mtl, cam)]
        if obj:
            register_textures(obj, mtl)
        c = _Cfg(width, height, shader, sceneIndex, samplesPixel, samplesLight, maxDepth, *self._keep, accelerator)
        self._h = lib().oracle_create(ctypes.byref(c))
        if not self._h:
            raise RuntimeError("oracle could not load the scene")

    def set_faithful(self, on=True):
        """Timing-faithful draws: the reference's shared atomic sampler cursors (results then
        depend on thread scheduling, as the reference's do)."""
        lib().oracle_set_faithful(self._h, int(on))

    def set_pixel_value(self, value=0.5):
        """The Constant pixel sampler's value of 1 spp frames and camera rays (the reference's: 0.5)."""
        lib().oracle_set_pixel_value(self._h, float(value))

    def num_tiles(self):
        return lib().oracle_num_tiles(self._h)

    def render(self, bitmap=None, threads=1, first_tile=0, num_tiles=1 << 30):
        if bitmap is None:
            bitmap = np.zeros(self.width * self.height, np.int32)
        rays = lib().oracle_render(self._h, bitmap.ctypes.data, threads, first_tile, num_tiles)
        return bitmap, int(rays)

    def render_tiles(self, tiles, bitmap=None, threads=1):
        if bitmap is None:
            bitmap = np.zeros(self.width * self.height, np.int32)
        t = np.ascontiguousarray(np.asarray(tiles, np.int32))
        rays = lib().oracle_render_tiles(self._h, bitmap.ctypes.data, threads, t.ctypes.data, len(t))
        return bitmap, int(rays)

    def counts(self):
        out = np.zeros(6, np.int64)
        lib().oracle_counts(self._h, out.ctypes.data)
        return dict(zip(("triangles", "lights", "planes", "spheres", "materials", "triangleNodes"), out.tolist()))

    def primary_hits(self):
        n = self.width * self.height
        k, i, t = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float32)
        lib().oracle_primary_hits(self._h, k.ctypes.data, i.ctypes.data, t.ctypes.data)
        return k, i, t

    def trace_rays(self, orig, dirs, dist=None, src=None, any_hit=False):
        """Closest hit (kind, input index, t) or, with any_hit, occlusion within dist of arbitrary
        rays; src: (n, 2) int32 (kind, input index) of each ray's source primitive, or None."""
        o = np.ascontiguousarray(orig, np.float32)
        d = np.ascontiguousarray(dirs, np.float32)
        n = len(o)
        ds = np.ascontiguousarray(dist if dist is not None else np.zeros(n), np.float32)
        sp = None if src is None else np.ascontiguousarray(src, np.int32)
        k, i, t = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float32)
        lib().oracle_trace_rays(self._h, o.ctypes.data, d.ctypes.data, ds.ctypes.data,
                                None if sp is None else sp.ctypes.data, n, int(any_hit),
                                k.ctypes.data, i.ctypes.data, t.ctypes.data)
        return k, i, t

    def shade_rays(self, orig, dirs, keys=None, src=None, threads=1):
        """Shader::rayTrace's rgb, before any conversion, of arbitrary rays: (rgb float32 (n, 3), rays
        cast).  Ray i is the depth-1 ray of a path with key keys[i] (None: path_key(i, 0)); src as for
        trace_rays.  The count includes the n given rays, as a frame's includes its camera rays."""
        o = np.ascontiguousarray(orig, np.float32)
        d = np.ascontiguousarray(dirs, np.float32)
        n = len(o)
        assert o.shape == (n, 3) and d.shape == (n, 3)
        ks = None if keys is None else np.ascontiguousarray(keys).astype(np.int64).astype(np.uint32)
        sp = None if src is None else np.ascontiguousarray(src, np.int32)
        assert (ks is None or ks.shape == (n,)) and (sp is None or sp.shape == (n, 2))
        rgb = np.zeros((n, 3), np.float32)
        casts = lib().oracle_shade_rays(self._h, o.ctypes.data, d.ctypes.data, None if ks is None else ks.ctypes.data,
                                        None if sp is None else sp.ctypes.data, n, int(threads), rgb.ctypes.data)
        return rgb, int(casts)

    def camera_rays(self, sample_base=0, spp=None):
        """The frame's camera rays (the engine's cameraRay) as (orig (n, 3), dirs (n, 3) float32, keys
        uint32, pixels int32): tiles in order, the pixels of a tile, samples sample_base ..
        sample_base + spp - 1 innermost (spp None: samplesPixel).  A pixel that two tiles cover
        appears once per tile."""
        spp = int(spp) if spp else max(1, self.samples_pixel)
        n = lib().oracle_camera_rays(self._h, int(sample_base), spp, None, None, None, None)
        o, d = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        keys, pixels = np.empty(n, np.uint32), np.empty(n, np.int32)
        lib().oracle_camera_rays(self._h, int(sample_base), spp, o.ctypes.data, d.ctypes.data, keys.ctypes.data,
                                 pixels.ctypes.data)
        return o, d, keys, pixels

    def triangle_bvh(self):
        n = lib().oracle_triangle_bvh(self._h, None, None, None, None)
        nt = self.counts()["triangles"]
        boxes = np.empty((n, 6), np.float32)
        off, cnt, order = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(nt, np.int32)
        lib().oracle_triangle_bvh(self._h, boxes.ctypes.data, off.ctypes.data, cnt.ctypes.data, order.ctypes.data)
        return boxes, off, cnt, order

    def regular_grid(self, kind):
        """RegularGrid of kind 0 planes / 1 spheres / 2 triangles (engine built with accelerator 2):
        world (12 floats: min, max, cellSize, cellSizeInverted), start (32^3 + 1), items (input
        indices)."""
        n = lib().oracle_regular_grid(self._h, kind, None, None, None)
        if n < 0:
            raise RuntimeError("the engine has no regular grid (accelerator != 2)")
        world, start, items = np.empty(12, np.float32), np.empty(32 ** 3 + 1, np.int32), np.empty(max(n, 1), np.int32)
        lib().oracle_regular_grid(self._h, kind, world.ctypes.data, start.ctypes.data, items.ctypes.data)
        return world, start, items[:n]

    def close(self):
        if getattr(self, "_h", None):
            lib().oracle_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


def kat_triangle(a, b, c, orig, direction, from_self=False):
    t = ctypes.c_float()
    hit = lib().oracle_kat_triangle(fvec(*a), fvec(*b), fvec(*c), fvec(*orig), fvec(*direction), int(from_self),
                                    ctypes.byref(t))
    return bool(hit), t.value


def grid_box_test(kind, prim, box):
    """Cell membership test of the RegularGrid fill: kind 0 prim = A + B + C, 1 = point + normal,
    2 = center + (radius,); box = min + max."""
    return bool(lib().oracle_grid_box_test(kind, fvec(*prim), fvec(*box)))


def kat_aabb(mn, mx, orig, direction):
    return bool(lib().oracle_kat_aabb(fvec(*mn), fvec(*mx), fvec(*orig), fvec(*direction)))


def aabb_props(mn, mx):
    c, a = fvec(0, 0, 0), ctypes.c_float()
    lib().oracle_aabb_props(fvec(*mn), fvec(*mx), c, ctypes.byref(a))
    return tuple(c), a.value


def triangle_aabb(a, b, c):
    mn, mx = fvec(0, 0, 0), fvec(0, 0, 0)
    lib().oracle_triangle_aabb(fvec(*a), fvec(*b), fvec(*c), mn, mx)
    return tuple(mn), tuple(mx)


def kat_plane(point, normal, orig, direction):
    t = ctypes.c_float()
    hit = lib().oracle_kat_plane(fvec(*point), fvec(*normal), fvec(*orig), fvec(*direction), ctypes.byref(t))
    return bool(hit), t.value


def kat_sphere(center, radius, orig, direction):
    t = ctypes.c_float()
    hit = lib().oracle_kat_sphere(fvec(*center), float(radius), fvec(*orig), fvec(*direction), ctypes.byref(t))
    return bool(hit), t.value


def plane_aabb(point, normal):
    mn, mx = fvec(0, 0, 0), fvec(0, 0, 0)
    lib().oracle_plane_aabb(fvec(*point), fvec(*normal), mn, mx)
    return tuple(mn), tuple(mx)


def kat_camera(path, ratio):
    out = fvec(*([0] * 14))
    if not lib().oracle_kat_camera(path.encode(), ratio, out):
        raise RuntimeError("camera file not parsed")
    v = list(out)
    return dict(position=v[0:3], direction=v[3:6], up=v[6:9], right=v[9:12], hfov=v[12], vfov=v[13])


def halton(index, base=2):
    return lib().oracle_halton(index, base)


def table(seed):
    out = np.empty(1 << 20, np.float32)
    lib().oracle_table(seed, out.ctypes.data)
    return out


def hemisphere_trig():
    out = np.empty(2 << 20, np.float32)
    lib().oracle_hemisphere_trig(out.ctypes.data)
    return out


def path_key(pixel, sample):
    return lib().oracle_path_key(pixel, sample)


def sample_index(key, tc, purpose):
    return lib().oracle_sample_index(key, tc, purpose)


def incremental_avg(rgb, avg, n):
    return lib().oracle_incremental_avg(rgb[0], rgb[1], rgb[2], avg, n)


def fast_arctan(v):
    return lib().oracle_fast_arctan(v)


def selftest_partition(seed=1, trials=2000):
    return lib().oracle_selftest_partition(seed, trials)
