"""Scenes that put the texture path (map_Kd: loadColor, textureWrite, the shared-Kd replay of
k_resolve; DESIGN.md deviation 4) where it can go wrong (tests only).  Everything is generated: the
images are written with the PNG encoder of test_texture_cpu.py.

* ``write_palette_scene``: small camera-facing triangles, each with ONE constant ``vt`` at the centre
  of a chosen texel, over five images of every channel count and odd sizes, so that a pixel's colour
  names the bytes that were read: the offset of the second and later textures in the shared texel
  array, the reads of a 1- or 2-channel image into the next texel, the clamp at the last texel.
* ``write_noise_scene``: quads mapped to random-noise images, with ``vt`` outside [0, 1) and the
  coordinates the loader's ``fract`` turns into exactly 1.0.
* ``write_corridor``: two facing mirrors with a texture each, where a vertex's subtree ends with a
  write to the OTHER material (and, with ``kt``, a glass slab whose transmission subtrees write both).
"""
import os

import numpy as np

from test_texture_cpu import _encode


def _q(x):  # snap to the 1/64 grid: exact in float32 and as short decimal text for every parser
    return round(x * 64.0) / 64.0


def _f(x):  # a float32 value as decimal text every correct parser reads back to the same float32
    return repr(float(np.float32(x)))


def write_png(path, samples, depth=8):
    """samples (h, w, channels) at `depth` bits -> a PNG of the colour type the channel count names."""
    samples = np.asarray(samples)
    ctype = {1: 0, 2: 4, 3: 2, 4: 6}[samples.shape[2]]
    with open(path, "wb") as f:
        f.write(_encode(samples, depth, ctype, rng=np.random.default_rng(samples.shape[0] * 131 + samples.shape[1])))


class _Obj:
    """Vertices, texture coordinates and triangles of an OBJ, written in face order."""

    def __init__(self):
        self.v, self.vt, self.faces = [], [], []  # faces: (material, ((v, vt) x 3))

    def tri(self, mat, pts, uvs):
        idx = []
        for p, t in zip(pts, uvs):
            self.v.append(p)
            self.vt.append(t)
            idx.append((len(self.v), len(self.vt)))
        self.faces.append((mat, tuple(idx)))
        return len(self.faces) - 1

    def quad(self, mat, a, b, c, d, ta, tb, tc, td):
        """Two triangles (c, b, a) and (d, c, a): the winding of extreme_scenes' quads."""
        return self.tri(mat, (c, b, a), (tc, tb, ta)), self.tri(mat, (d, c, a), (td, tc, ta))

    def write(self, path, mtllib):
        with open(path, "w") as f:
            f.write("mtllib %s\n" % mtllib)
            for p in self.v:
                f.write("v %s %s %s\n" % tuple(_f(c) for c in p))
            for t in self.vt:
                f.write("vt %s %s\n" % (t[0] if isinstance(t[0], str) else _f(t[0]),
                                        t[1] if isinstance(t[1], str) else _f(t[1])))
            last = None
            for mat, idx in self.faces:
                if mat != last:
                    f.write("usemtl %s\n" % mat)
                    last = mat
                f.write("f %d/%d %d/%d %d/%d\n" % (idx[0] + idx[1] + idx[2]))


# ---- the palette -------------------------------------------------------------------------------------
# material -> (image file, width, height, channels, bit depth); MTL order
PALETTE_IMAGES = {
    "m1": ("grey.png", 5, 3, 1, 8),
    "m2": ("greyalpha.png", 3, 5, 2, 8),
    "m3": ("rgb.png", 7, 1, 3, 8),
    "m4": ("rgba.png", 1, 1, 4, 8),
    "m5": ("rgb16.png", 4, 4, 3, 16),
}
PALETTE_KD = {  # the MTL's Kd: what an untextured hit, or a texture that is not there, shows
    "m1": (0.5, 0.5, 0.5), "m2": (0.5, 0.5, 0.5), "m3": (0.5, 0.5, 0.5), "m4": (0.5, 0.5, 0.5),
    "m5": (0.5, 0.5, 0.5), "m6": (0.25, 0.5, 0.75), "m7": (0.75, 0.25, 0.5), "m8": (0.125, 0.875, 0.375),
}
# material -> texels (i, j), two per quad: every corner, the last texel (the clamp), a texel of the
# last row for the 1- and 2-channel images, one inside
PALETTE_TEXELS = {
    "m1": [(0, 0), (4, 0), (0, 2), (4, 2), (2, 2), (3, 2), (2, 1), (1, 1)],
    "m2": [(0, 0), (2, 0), (0, 4), (2, 4), (1, 4), (1, 2)],
    "m3": [(0, 0), (6, 0), (3, 0), (5, 0)],
    "m4": [(0, 0), (0, 0)],
    "m5": [(0, 0), (3, 0), (0, 3), (3, 3), (1, 2), (2, 3)],
    "m6": [None, None],
    "m7": [(1, 1), (0, 0)],
    "m8": [(0, 0), (6, 0), (5, 0), (1, 0)],
}


def palette_samples():
    """material -> the samples written into its image, (h, w, channels) at the image's bit depth."""
    rng = np.random.default_rng(20240)
    out = {}
    for name, (_, w, h, ch, depth) in PALETTE_IMAGES.items():
        out[name] = rng.integers(1, 1 << depth, size=(h, w, ch))
    return out


def write_palette_scene(path):
    """Returns (obj, mtl, cam, table): table[k] = (material, image material or None, texel or None) of
    triangle k in input order (the index primary_hits reports); the last two triangles are the light."""
    os.makedirs(path, exist_ok=True)
    obj, mtl, cam = (os.path.join(path, "palette." + e) for e in ("obj", "mtl", "cam"))
    samples = palette_samples()
    for name, (file, _, _, _, depth) in PALETTE_IMAGES.items():
        write_png(os.path.join(path, file), samples[name], depth)
    image_of = {"m1": "m1", "m2": "m2", "m3": "m3", "m4": "m4", "m5": "m5", "m6": None, "m7": None, "m8": "m3"}
    with open(mtl, "w") as f:
        for name, kd in PALETTE_KD.items():
            f.write("newmtl %s\nKd %r %r %r\nKs 0 0 0\n" % ((name,) + kd))
            if name == "m7":
                f.write("map_Kd missing.png\n")
            elif image_of[name] is not None:
                f.write("map_Kd %s\n" % PALETTE_IMAGES[image_of[name]][0])
            f.write("\n")
        f.write("newmtl light\nKd 0.78 0.78 0.78\nKs 0 0 0\nKe 10 10 10\n")
    o = _Obj()
    table = []
    cells = [(name, PALETTE_TEXELS[name][k:k + 2]) for name in PALETTE_KD for k in range(0, len(PALETTE_TEXELS[name]), 2)]
    cols = 5
    cell, size = 1.5, 1.25
    for n, (name, pair) in enumerate(cells):
        x0 = _q(-0.5 * cols * cell + (n % cols) * cell + 0.5 * (cell - size))
        y0 = _q(-0.5 * 4 * cell + (n // cols) * cell + 0.5 * (cell - size))
        z = _q((n % 3) / 8.0)
        a, b, c, d = (x0, y0, z), (x0 + size, y0, z), (x0 + size, y0 + size, z), (x0, y0 + size, z)
        img = image_of[name]
        for pts, texel in (((c, b, a), pair[0]), ((d, c, a), pair[1])):
            if texel is None:
                uv = (0.5, 0.5)
            else:
                w, h = (PALETTE_IMAGES[img][1:3] if img is not None else (2, 2))
                uv = (np.float32(texel[0] + 0.5) / np.float32(w), np.float32(texel[1] + 0.5) / np.float32(h))
            o.tri(name, pts, (uv, uv, uv))
            table.append((name, img, texel if img is not None else None))
    lo, hi = -2.0, 2.0
    o.quad("light", (lo, 5.5, -4.0), (hi, 5.5, -4.0), (hi, 5.5, -2.0), (lo, 5.5, -2.0), *([(0.5, 0.5)] * 4))
    o.write(obj, "palette.mtl")
    with open(cam, "w") as f:
        f.write(palette_cam_text(0))
    return obj, mtl, cam, table


# two cameras of the palette scene: position, lookAt, (f.u, f.v) of the .cam file; exact in float32
PALETTE_CAMS = [((0.0, 0.0, -10.0), (0.0, 0.0, 0.0), (50.0, 50.0)),
                ((1.5, -0.75, -9.0), (0.25, 0.0, 0.0), (50.0, 50.0))]


def palette_cam_text(k):
    p, l, f = PALETTE_CAMS[k]
    return "t perspective\np %r %r %r\nl %r %r %r\nu 0 1 0\nf %r %r\n" % (*p, *l, *f)


def palette_views():
    """PALETTE_CAMS as Renderer.render_views takes them (what the loader makes of the .cam text at a
    square frame: position X negated, hFov = f.u * 1)."""
    return [(0, (-p[0], p[1], p[2]), l, (0.0, 1.0, 0.0), f[0], f[1]) for p, l, f in PALETTE_CAMS]


# ---- noise -------------------------------------------------------------------------------------------
def write_noise_scene(path):
    """Returns (obj, mtl, cam, quads): quads[name] = the input-order triangle indices of quad `name`
    ("wrap": vt outside [0, 1), "plain", "edge_u": tx == 1, "edge_uv": both coordinates 1)."""
    os.makedirs(path, exist_ok=True)
    obj, mtl, cam = (os.path.join(path, "noise." + e) for e in ("obj", "mtl", "cam"))
    rng = np.random.default_rng(53037)
    write_png(os.path.join(path, "noise_rgb.png"), rng.integers(0, 256, size=(37, 53, 3)))
    write_png(os.path.join(path, "noise_rgba.png"), rng.integers(0, 256, size=(16, 16, 4)))
    with open(mtl, "w") as f:
        f.write("newmtl a\nKd 0.5 0.5 0.5\nKs 0 0 0\nmap_Kd noise_rgb.png\n\n")
        f.write("newmtl b\nKd 0.5 0.5 0.5\nKs 0 0 0\nmap_Kd noise_rgba.png\n\n")
        f.write("newmtl light\nKd 0.78 0.78 0.78\nKs 0 0 0\nKe 10 10 10\n")
    o = _Obj()
    quads = {}
    eps = "-1e-8"  # fract(-1e-8f) == 1.0f exactly
    quads["wrap"] = o.quad("a", (-4.0, 0.25, 0.0), (-0.25, 0.25, 0.0), (-0.25, 4.0, 0.0), (-4.0, 4.0, 0.0),
                           (-0.25, 3.5), ("1.0", 3.5), ("1.0", eps), (-0.25, eps))
    quads["plain"] = o.quad("b", (0.25, 0.25, 0.125), (4.0, 0.25, 0.125), (4.0, 4.0, 0.125), (0.25, 4.0, 0.125),
                            (0.0, 0.0), (0.96875, 0.0), (0.96875, 0.96875), (0.0, 0.96875))
    quads["edge_u"] = o.quad("a", (-4.0, -4.0, 0.25), (-0.25, -4.0, 0.25), (-0.25, -0.25, 0.25), (-4.0, -0.25, 0.25),
                             *([(eps, 0.5)] * 4))
    quads["edge_uv"] = o.quad("b", (0.25, -4.0, 0.0), (4.0, -4.0, 0.0), (4.0, -0.25, 0.0), (0.25, -0.25, 0.0),
                              *([(eps, eps)] * 4))
    o.quad("light", (-2.0, 5.5, -4.0), (2.0, 5.5, -4.0), (2.0, 5.5, -2.0), (-2.0, 5.5, -2.0), *([(0.5, 0.5)] * 4))
    o.write(obj, "noise.mtl")
    with open(cam, "w") as f:
        f.write("t perspective\np 0 0 -10\nl 0 0 0\nu 0 1 0\nf 50 50\n")
    return obj, mtl, cam, quads


# ---- the corridor --------------------------------------------------------------------------------------
CORRIDOR = dict(x0=-4.0, x1=4.0, z0=-4.0, z1=12.0, strips=8, top=0.96875)
CORRIDOR_IMAGES = {"X": ("x.png", 16, 16), "Y": ("y.png", 11, 13)}  # file, width, height


def corridor_texel(name, x, z):
    """The texel of image `name` under the file-space point (x, z) of the floor (X) or ceiling (Y), in
    float64 (for tests that only ask whether two hits see different texels)."""
    c = CORRIDOR
    _, w, h = CORRIDOR_IMAGES[name]
    depth = (c["z1"] - c["z0"]) / c["strips"]
    fz = ((z - c["z0"]) % depth) / depth
    if name == "Y":  # the ceiling's strips run from z1 down
        fz = ((c["z1"] - z) % depth) / depth
    fx = (x - c["x0"]) / (c["x1"] - c["x0"])
    return int(fx * c["top"] * w), int(fz * c["top"] * h)


def write_corridor(path, textured=("X", "Y"), kt=False):
    """Floor y = -0.5 (material X) and ceiling y = +0.5 (material Y), both Kd 1 1 1 and Ks 0.5, over
    x in [-4, 4], z in [-4, 12], in strips whose ``vt`` each span one repeat of the image (strip k:
    v from k to k + 31/32, which the loader wraps); emissive side walls; with `kt` material X also
    transmits (Tf, d 0.5, Ni 1.5) and a tilted slab of it stands across the corridor.
    Returns (obj, mtl, cam, tris): tris[name] = the input-order triangle indices of "X", "Y", "slab"."""
    os.makedirs(path, exist_ok=True)
    obj, mtl, cam = (os.path.join(path, "corridor." + e) for e in ("obj", "mtl", "cam"))
    rng = np.random.default_rng(7)
    for name, (file, w, h) in CORRIDOR_IMAGES.items():
        write_png(os.path.join(path, file), rng.integers(1, 256, size=(h, w, 3)))
    with open(mtl, "w") as f:
        # with `kt` material X transmits: the slab's (and the floor's) hits have a T subtree
        f.write("newmtl X\nKd 1 1 1\nKs 0.5 0.5 0.5\n%s%s\n" % ("Tf 0.75 0.75 0.75\nd 0.5\nNi 1.5\n" if kt else "",
                                                              "map_Kd x.png\n" if "X" in textured else ""))
        f.write("newmtl Y\nKd 1 1 1\nKs 0.5 0.5 0.5\n%s\n" % ("map_Kd y.png\n" if "Y" in textured else ""))
        f.write("newmtl light\nKd 0.78 0.78 0.78\nKs 0 0 0\nKe 10 10 10\n")
    o = _Obj()
    tris = {"X": (), "Y": ()}
    c = CORRIDOR
    x0, x1, z0, z1, top = c["x0"], c["x1"], c["z0"], c["z1"], c["top"]
    depth = (z1 - z0) / c["strips"]
    for k in range(c["strips"]):
        za, zb = z0 + k * depth, z0 + (k + 1) * depth
        tris["X"] += o.quad("X", (x0, -0.5, za), (x1, -0.5, za), (x1, -0.5, zb), (x0, -0.5, zb),
                            (0.0, float(k)), (top, float(k)), (top, k + top), (0.0, k + top))
    for k in range(c["strips"]):
        za, zb = z1 - k * depth, z1 - (k + 1) * depth
        tris["Y"] += o.quad("Y", (x0, 0.5, za), (x1, 0.5, za), (x1, 0.5, zb), (x0, 0.5, zb),
                            (0.0, -float(k)), (top, -float(k)), (top, -k + top), (0.0, -k + top))
    if kt:  # tilted, so that its reflections and refractions reach both mirrors
        tris["slab"] = o.quad("X", (x0, -0.5, 1.0), (x1, -0.5, 1.0), (x1, 0.5, 1.5), (x0, 0.5, 1.5),
                              (0.0, 0.0), (top, 0.0), (top, 2.0 + top), (0.0, 2.0 + top))
    half = [(0.5, 0.5)] * 4
    # emissive side walls, in several quads (so that a frame is lit under the PathTracer too, whose
    # every vertex samples one light)
    for k in range(4):
        za, zb = z0 + 4.0 * k, z0 + 4.0 * k + 4.0
        o.quad("light", (x0, -0.5, zb), (x0, -0.5, za), (x0, 0.5, za), (x0, 0.5, zb), *half)
        o.quad("light", (x1, -0.5, za), (x1, -0.5, zb), (x1, 0.5, zb), (x1, 0.5, za), *half)
    o.write(obj, "corridor.mtl")
    with open(cam, "w") as f:
        f.write("t perspective\np 0 0 -3.5\nl 0 -0.6 -2.5\nu 0 1 0\nf 60 60\n")
    return obj, mtl, cam, tris
