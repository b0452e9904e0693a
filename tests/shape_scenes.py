"""Scenes whose triangle list alone decides which walk runs (tests only): the depth of the reference
tree (the packet walk's stack limit, the per-lane walks' spill stacks), zero-area triangles in the
leaves of real ones, and boxes that are not finite (no quantized walk tree).

Every scene is the same base - a lit floor and back wall, a grid of camera-facing quads (every third
tilted, so that their boxes have a volume) with a few specular and transmissive materials, one area
light overhead that faces them - plus what its name says.  Everything is generated; every coordinate
is exact in float32 and written as decimal text that every correct parser reads back to it.
"""
import os

import numpy as np

from extreme_scenes import _q, material_kd

BASE_LO, BASE_HI = (-8.0, -5.0, -10.0), (8.0, 5.0, 3.0)  # the room: the base's floor and walls (file coordinates)
LIGHT_Y = 9.0
GRID = 6  # the base's quads: GRID x GRID

# stack(n): n coincident copies.  Beside each n: the reference tree's depth (the oracle's build) and
# the walk's stack need (mrt_walk_stack), measured on the host; the packet walk takes need <= 128.
# The need is the larger of the binary walk tree's depth + 2 and 3 * (levels of the wide walk tree) + 2;
# no n gives 127 or 130.
STACK_CASES = {
    # n: (reference depth, stack need)
    9: (9, 17),         # packet walk
    130: (105, 126),    # packet walk
    132: (107, 128),    # packet walk: the limit itself
    133: (108, 129),    # per-lane walk: one entry too many
    135: (110, 131),    # per-lane walk
    450: (425, 446),    # per-lane walk, 438 spill entries per thread
}
STACK_DEEP = 450
# the other scenes: degenerate (9, 14), outlier (9, 14): packet walk; inf_vertex and overflow
# (81, 83): not quantized, every ray walks the reference tree in the reference's order

SCENES = ("degenerate", "inf_vertex", "overflow", "outlier")
NON_FINITE = ("inf_vertex", "overflow")


def _f(x):
    """A float32 value as decimal text (a string is written as it stands)."""
    return x if isinstance(x, str) else repr(float(np.float32(x)))


class _Mesh:
    def __init__(self):
        self.v, self.faces = [], []  # faces: (material, vertex indices)

    def quad(self, mat, a, b, c, d):
        k = len(self.v)
        self.v.extend([a, b, c, d])
        self.faces.append((mat, (k + 4, k + 3, k + 2, k + 1)))  # (the loader fans it: two triangles)
        return 2

    def tri(self, mat, a, b, c):
        k = len(self.v)
        self.v.extend([a, b, c])
        self.faces.append((mat, (k + 3, k + 2, k + 1)))
        return 1

    def write(self, path, mtllib):
        with open(path, "w") as f:
            f.write("mtllib %s\n" % mtllib)
            for p in self.v:
                f.write("v %s %s %s\n" % tuple(_f(c) for c in p))
            last = None
            for mat, idx in self.faces:
                if mat != last:
                    f.write("usemtl %s\n" % mat)
                    last = mat
                f.write("f " + " ".join("%d" % i for i in idx) + "\n")


def _grid_quad(i):
    """Corners a, b, c, d of the base's quad i (counter-clockwise seen from the camera)."""
    cell, size = 1.25, 1.0
    x0 = -0.5 * GRID * cell + (i % GRID) * cell
    y0 = -0.5 * GRID * cell + (i // GRID) * cell
    z = _q(-(i % 5) / 8.0)
    dz = (i % 3 - 1) * 0.25  # every third leans left, every third right
    return (x0, y0, z), (x0 + size, y0, z + dz), (x0 + size, y0 + size, z + dz), (x0, y0 + size, z)


def _base(mesh, mtl_file):
    """The base scene into `mesh` and its materials into the open MTL; returns its triangle count."""
    mtl_file.write("newmtl floor\nKd 0.75 0.75 0.75\nKs 0 0 0\n\n")
    mtl_file.write("newmtl wall\nKd 0.5 0.25 0.75\nKs 0 0 0\n\n")
    for i in range(GRID * GRID):
        mtl_file.write("newmtl g%d\nKd %r %r %r\n" % ((i,) + material_kd(100 + 37 * i)))
        mtl_file.write("Ks 0.25 0.25 0.25\n" if i % 4 == 0 else "Ks 0 0 0\n")
        if i % 7 == 3:
            mtl_file.write("Tf 0.6 0.6 0.6\nd 0.5\nNi 1.5\n")
        mtl_file.write("\n")
    mtl_file.write("newmtl light\nKd 0.78 0.78 0.78\nKs 0 0 0\nKe 10 10 10\n\n")
    n = mesh.quad("floor", (-8, -5, -10), (8, -5, -10), (8, -5, 3), (-8, -5, 3))
    n += mesh.quad("wall", (-8, -5, 2), (8, -5, 2), (8, 5, 2), (-8, 5, 2))
    # side walls: most rays from inside the room hit something
    n += mesh.quad("wall", (-8, -5, -10), (-8, -5, 3), (-8, 5, 3), (-8, 5, -10))
    n += mesh.quad("wall", (8, -5, 3), (8, -5, -10), (8, 5, -10), (8, 5, 3))
    for i in range(GRID * GRID):
        n += mesh.quad("g%d" % i, *_grid_quad(i))
    return n


def _light(mesh):
    """The area light, written last (the loader keeps emissive triangles out of the triangle list, so
    every other triangle's input index is its position among the non-emissive ones).  It lies above
    every surface and every origin of the tests' random rays: a ray that hits it travels upward and
    never reaches what a scene adds below the floor."""
    mesh.quad("light", (-3, LIGHT_Y, -7), (3, LIGHT_Y, -7), (3, LIGHT_Y, -1), (-3, LIGHT_Y, -1))


def _paths(path, name):
    os.makedirs(path, exist_ok=True)
    return tuple(os.path.join(path, name + "." + e) for e in ("obj", "mtl", "cam"))


def _cam(cam):
    with open(cam, "w") as f:
        f.write("t perspective\np 0 0 -10\nl 0 0 0\nu 0 1 0\nf 60 60\n")


def write_base(path):
    obj, mtl, cam = _paths(path, "base")
    mesh = _Mesh()
    with open(mtl, "w") as f:
        _base(mesh, f)
    _light(mesh)
    mesh.write(obj, "base.mtl")
    _cam(cam)
    return obj, mtl, cam


def write_stack(path, n):
    """The base plus `n` coincident copies of one camera-facing triangle in front of the grid, copy k
    with the material s<k> of Kd material_kd(k).  Returns (obj, mtl, cam, first): the copies are the
    input triangles first .. first + n - 1."""
    obj, mtl, cam = _paths(path, "stack%d" % n)
    mesh = _Mesh()
    with open(mtl, "w") as f:
        first = _base(mesh, f)
        for k in range(n):
            f.write("newmtl s%d\nKd %r %r %r\nKs 0 0 0\n\n" % ((k,) + material_kd(k)))
    for k in range(n):
        mesh.tri("s%d" % k, (-2.5, -2.0, -2.0), (2.5, -2.0, -2.0), (0.5, 2.5, -2.0))
    _light(mesh)
    mesh.write(obj, os.path.basename(mtl))
    _cam(cam)
    return obj, mtl, cam, first


def write_degenerate(path):
    """The base plus zero-area triangles: points (three identical vertices), segments (two identical),
    collinear triples and needles whose area underflows, on the corners, on the edges and inside the
    boxes of the grid's quads, a few alone in empty space and a few on the camera's axis.
    Returns (obj, mtl, cam, first): the zero-area triangles are the input triangles from `first` on."""
    obj, mtl, cam = _paths(path, "degenerate")
    mesh = _Mesh()
    with open(mtl, "w") as f:
        first = _base(mesh, f)
        f.write("newmtl zero\nKd 1 0 0\nKs 0.5 0.5 0.5\n\n")
    tiny = 2.0 ** -80  # tiny * tiny underflows to 0 in float32

    def mid(p, q, w=0.5):
        return tuple(_q(p[k] + w * (q[k] - p[k])) for k in range(3))

    def point(p):
        mesh.tri("zero", p, p, p)

    def segment(p, q):
        mesh.tri("zero", p, p, q)

    def collinear(p, q):
        mesh.tri("zero", p, mid(p, q), q)

    def needle(p, up=1):  # legs along x and axis `up` from coordinates that are 0 (0 + tiny is exact)
        q = list(p)
        q[up] += tiny
        mesh.tri("zero", p, (p[0] + tiny, p[1], p[2]), tuple(q))

    for i in range(GRID * GRID):
        a, b, c, d = _grid_quad(i)
        centre = mid(a, c)
        kind = i % 6
        if kind == 0:      # on a corner, and a segment along an edge
            point(a)
            segment(a, b)
        elif kind == 1:    # collinear along the diagonal the two triangles share; a point on an edge
            collinear(a, c)
            point(mid(b, c))
        elif kind == 2:    # inside the boxes, off the plane where the quad leans
            point((centre[0], centre[1], a[2]))
            collinear(mid(a, b, 0.25), mid(d, c, 0.75))
        elif kind == 3:    # a segment across the quad, corner to corner
            segment(b, d)
            point(c)
        elif kind == 4:    # two coincident points and a segment standing on the quad
            point(centre)
            point(centre)
            segment(centre, (centre[0], centre[1], centre[2] - 0.25))
        else:
            collinear(d, c)
            segment(mid(a, d), mid(b, c))
    # needles: two on the camera's axis, one in the floor
    needle((0.0, 0.0, -2.0))
    needle((0.0, 0.0, 0.0))
    needle((0.0, -5.0, 0.0), up=2)
    # the camera's axis (x = y = 0): a point, a segment along it, a collinear triple across it
    point((0.0, 0.0, -5.0))
    segment((0.0, 0.0, -6.0), (0.0, 0.0, -4.0))
    collinear((-1.0, 0.0, -3.0), (1.0, 0.0, -3.0))
    # alone in empty space
    point((6.0, 3.0, -3.0))
    segment((-6.0, 4.0, -4.0), (-5.0, 4.5, -3.0))
    collinear((5.0, -3.0, -6.0), (7.0, -1.0, -4.0))
    _light(mesh)
    mesh.write(obj, os.path.basename(mtl))
    _cam(cam)
    return obj, mtl, cam, first


def _write_plus(path, name, tris):
    obj, mtl, cam = _paths(path, name)
    mesh = _Mesh()
    with open(mtl, "w") as f:
        first = _base(mesh, f)
        f.write("newmtl extra\nKd 0.25 0.75 0.5\nKs 0 0 0\n\n")
    for tri in tris:
        mesh.tri("extra", *tri)
    _light(mesh)
    mesh.write(obj, os.path.basename(mtl))
    _cam(cam)
    return obj, mtl, cam, first


# Where the non-finite scenes put their triangles: far below the floor (y <= -9: below every origin
# of the tests' random rays too), under and beyond the back of the room.  A non-finite triangle's
# test returns a NaN t for every ray that reaches it, which the reference accepts (Triangle.cpp:104);
# the answer then depends on the reference's visit order, and a light accepted after it has no
# material, which the reference dereferences (AreaLight.cpp:35-39, Shader.cpp:122).  Only rays that
# travel downward past the floor reach a leaf down here, and none of them hits the light above.  Three
# finite triangles follow the non-finite one: the reference's build, whose SAH has no finite area to
# compare on such input, peels single triangles off in input order and leaves the last four as one
# leaf, so that leaf holds these four and nothing of the room (tests/test_tree_shapes.py asserts it).
_BELOW = [((-8.0, -9.0, 2.5), (8.0, -12.0, 2.5), (8.0, -9.0, 40.0)),
          ((-8.0, -10.0, 3.0), (-8.0, -12.0, 40.0), (8.0, -11.0, 40.0)),
          ((0.0, -9.5, 5.0), (2.0, -9.5, 5.0), (1.0, -10.5, 9.0))]


def write_inf_vertex(path):
    """The base plus one triangle with a vertex coordinate written 1e39, which parses to infinity (and
    three finite ones beside it, see _BELOW).  The non-finite one is the input triangle `first`."""
    return _write_plus(path, "inf_vertex", _BELOW + [(("1e39", -9.0, 2.5), (8.0, -12.0, 2.5), (8.0, -9.0, 40.0))])


def write_overflow(path):
    """The base plus one triangle whose vertices are finite but whose edges A -> B, A -> C and box
    extent overflow (and three ordinary ones beside it, see _BELOW)."""
    return _write_plus(path, "overflow", _BELOW + [((3e38, -9.0, 2.5), (-3e38, -12.0, 2.5), (3e38, -9.0, 40.0))])


def write_outlier(path):
    """The base plus one small triangle at (2^40, 2^40, 2^40): one step of the walk tree's 16-bit grid
    is then larger than the rest of the scene."""
    p, e = 2.0 ** 40, 2.0 ** 18
    return _write_plus(path, "outlier", [((p, p, p), (p + e, p, p), (p, p + e, p + e))])


def write_scene(path, name):
    """(obj, mtl, cam, first) of "base", "stack<n>" or a name of SCENES."""
    if name == "base":
        return write_base(path) + (None,)
    if name.startswith("stack"):
        return write_stack(path, int(name[5:]))
    return {"degenerate": write_degenerate, "inf_vertex": write_inf_vertex, "overflow": write_overflow,
            "outlier": write_outlier}[name](path)
