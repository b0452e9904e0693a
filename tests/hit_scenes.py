"""A small room for the surface records of the ray queries (tests only): every kind of triangle the
records distinguish, in one OBJ whose coordinates, normals and texture coordinates are on the 1/64 grid
(exact in float32 and as short decimal text).

* floor and ceiling: flat (no ``vn``), untextured (``plain``);
* left wall: flat, textured (``tex``, ``vt`` inside [0, 1));
* back wall: smooth (explicit ``vn`` that differ at every corner), textured;
* right wall: smooth, untextured (``blue``);
* an octahedron: smooth, ``gloss`` (Kd 0, Ks and Kt set, Ni 1.5);
* two tilted corner panels: flat with a normal that is no axis (``blue``);
* one emissive quad under the ceiling (``light``, Ke above 1: the loader normalises it);
* the front (file z = -2) is open: the camera of the ``.cam`` looks in through it.

The walls are split 2 x 2, so the room has 50 triangles and 2 lights.
"""
import os

import numpy as np

from texture_scenes import _f, write_png

X0, X1, Y0, Y1, Z0, Z1 = -2.0, 2.0, -1.5, 1.5, -2.0, 2.0

# what the MTL says, and what the loader makes of it (Kt = Tf * (1 - d), Le = Ke / max(Ke) above 1)
MATERIALS = {
    "plain": dict(kd=(0.75, 0.75, 0.75), ks=(0.0, 0.0, 0.0), kt=(0.0, 0.0, 0.0), le=(0.0, 0.0, 0.0), ior=1.0, image=None),
    "blue": dict(kd=(0.25, 0.5, 0.75), ks=(0.0, 0.0, 0.0), kt=(0.0, 0.0, 0.0), le=(0.0, 0.0, 0.0), ior=1.0, image=None),
    "tex": dict(kd=(0.5, 0.5, 0.5), ks=(0.0, 0.0, 0.0), kt=(0.0, 0.0, 0.0), le=(0.0, 0.0, 0.0), ior=1.0, image="room.png"),
    "gloss": dict(kd=(0.0, 0.0, 0.0), ks=(0.5, 0.5, 0.5), kt=(0.375, 0.375, 0.375), le=(0.0, 0.0, 0.0), ior=1.5, image=None),
    "light": dict(kd=(0.0, 0.0, 0.0), ks=(0.0, 0.0, 0.0), kt=(0.0, 0.0, 0.0), le=(1.0, 0.5, 0.25), ior=1.0, image=None),
}
MTL_TEXT = """newmtl plain
Kd 0.75 0.75 0.75
Ks 0 0 0

newmtl blue
Kd 0.25 0.5 0.75
Ks 0 0 0

newmtl tex
Kd 0.5 0.5 0.5
Ks 0 0 0
map_Kd room.png

newmtl gloss
Kd 0 0 0
Ks 0.5 0.5 0.5
Tf 0.75 0.75 0.75
d 0.5
Ni 1.5

newmtl light
Kd 0 0 0
Ks 0 0 0
Ke 8 4 2
"""
CAM_TEXT = "t perspective\np 0 0 -4.5\nl 0 0 0\nu 0 1 0\nf 50 50\n"
IMAGE_SIZE = (8, 8)  # width, height of room.png


class _Room:
    """Vertices, texture coordinates, normals and triangles of an OBJ, written in face order; a
    corner is (point, vt or None, vn or None)."""

    def __init__(self):
        self.v, self.vt, self.vn, self.faces = [], [], [], []

    def tri(self, mat, corners):
        idx = []
        for p, t, n in corners:
            self.v.append(p)
            vt = vn = 0
            if t is not None:
                self.vt.append(t)
                vt = len(self.vt)
            if n is not None:
                self.vn.append(n)
                vn = len(self.vn)
            idx.append((len(self.v), vt, vn))
        self.faces.append((mat, corners, idx))

    def quad(self, mat, a, b, c, d):
        """Two triangles (c, b, a) and (d, c, a) of the corners a, b, c, d."""
        self.tri(mat, (c, b, a))
        self.tri(mat, (d, c, a))

    def write(self, path, mtllib):
        with open(path, "w") as f:
            f.write("mtllib %s\n" % mtllib)
            for p in self.v:
                f.write("v %s %s %s\n" % tuple(_f(c) for c in p))
            for t in self.vt:
                f.write("vt %s %s\n" % tuple(_f(c) for c in t))
            for n in self.vn:
                f.write("vn %s %s %s\n" % tuple(_f(c) for c in n))
            last = None
            for mat, _, idx in self.faces:
                if mat != last:
                    f.write("usemtl %s\n" % mat)
                    last = mat
                f.write("f %s\n" % " ".join(
                    "%d/%d/%d" % (v, t, n) if t and n else "%d//%d" % (v, n) if n else "%d/%d" % (v, t) if t else "%d" % v
                    for v, t, n in idx))


def _wall(room, mat, origin, du, dv, uv=False, normal=None):
    """A wall origin + s du + t dv (s, t in [0, 1]) as 2 x 2 quads.  uv: vt = (s, t) * 31/32; normal: a
    function (s, t) -> vn of the corner."""
    def corner(s, t):
        p = tuple(origin[k] + s * du[k] + t * dv[k] for k in range(3))
        return p, ((s * 0.96875, t * 0.96875) if uv else None), (normal(s, t) if normal else None)
    for i in range(2):
        for j in range(2):
            s0, s1, t0, t1 = i / 2.0, (i + 1) / 2.0, j / 2.0, (j + 1) / 2.0
            room.quad(mat, corner(s0, t0), corner(s1, t0), corner(s1, t1), corner(s0, t1))


def write_room(path):
    """Returns (obj, mtl, cam, table): table[k] describes triangle k of the loaded scene, in input order
    (the emissive quad is no triangle of the scene: it becomes two lights) - ``material`` (the MTL
    name), ``smooth`` (explicit normals), ``vn`` (the three normals as written, or None), ``textured``."""
    os.makedirs(path, exist_ok=True)
    obj, mtl, cam = (os.path.join(path, "room." + e) for e in ("obj", "mtl", "cam"))
    rng = np.random.default_rng(8128)
    write_png(os.path.join(path, "room.png"), rng.integers(1, 256, size=(IMAGE_SIZE[1], IMAGE_SIZE[0], 3)))
    with open(mtl, "w") as f:
        f.write(MTL_TEXT)
    with open(cam, "w") as f:
        f.write(CAM_TEXT)
    r = _Room()
    w, h, d = X1 - X0, Y1 - Y0, Z1 - Z0
    _wall(r, "plain", (X0, Y0, Z0), (w, 0.0, 0.0), (0.0, 0.0, d))                       # floor
    _wall(r, "plain", (X0, Y1, Z0), (w, 0.0, 0.0), (0.0, 0.0, d))                       # ceiling
    _wall(r, "tex", (X0, Y0, Z0), (0.0, 0.0, d), (0.0, h, 0.0), uv=True)                # left: flat, textured
    _wall(r, "tex", (X0, Y0, Z1), (w, 0.0, 0.0), (0.0, h, 0.0), uv=True,               # back: smooth, textured
          normal=lambda s, t: (0.5 * (s - 0.5), 0.5 * (t - 0.5), -1.0))
    _wall(r, "blue", (X1, Y0, Z0), (0.0, 0.0, d), (0.0, h, 0.0),                        # right: smooth
          normal=lambda s, t: (-1.0, 0.5 * (t - 0.5), 0.25 * (s - 0.5) + 0.125))
    # the octahedron: each corner's normal points away from the centre
    c, e = (0.5, -0.5, 0.5), 0.5
    tip = {k: (tuple(c[a] + (e if a == k[1] else 0.0) * k[0] for a in range(3)),
               tuple(float(k[0]) if a == k[1] else 0.0 for a in range(3))) for k in
           ((1, 0), (-1, 0), (1, 1), (-1, 1), (1, 2), (-1, 2))}
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                r.tri("gloss", tuple((tip[k][0], None, tip[k][1]) for k in ((sx, 0), (sy, 1), (sz, 2))))
    # two flat panels across the back corners of the floor: their normals are no axis
    r.tri("blue", (((X0, Y0, 1.0), None, None), ((-1.0, Y0, Z1), None, None), ((X0, -0.5, Z1), None, None)))
    r.tri("blue", (((X1, Y0, 1.25), None, None), ((1.0, Y0, Z1), None, None), ((X1, -0.75, Z1), None, None)))
    y = Y1 - 1.0 / 64.0
    r.quad("light", ((-1.0, y, -1.0), None, None), ((1.0, y, -1.0), None, None), ((1.0, y, 1.0), None, None),
           ((-1.0, y, 1.0), None, None))
    r.write(obj, "room.mtl")
    table = []
    for mat, corners, _ in r.faces:
        if mat == "light":
            continue
        smooth = corners[0][2] is not None
        table.append(dict(material=mat, smooth=smooth, vn=[n for _, _, n in corners] if smooth else None,
                          textured=MATERIALS[mat]["image"] is not None))
    return obj, mtl, cam, table
