"""The cases of the reference fixtures (tests/golden/reference/): what tests/golden/make_reference_fixtures.py
records with the reference's own code, and what tests/test_reference_fixtures_{cpu,gpu}.py hold the oracle
and the kernels to.  Tests only.

Every generated input comes from numpy's legacy ``RandomState``, whose streams never change, or from a
formula; the manifest holds the SHA-256 of every input, so an input that a test rebuilds here (the
known-answer cases, the camera rows, the conversion rows: large and of full entropy) is checked against
what the reference was given before it is used.  The mesh rays are stored with their results.
"""
import hashlib
import io
import json
import os
import zipfile

import numpy as np

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
FIXTURES = os.path.join(GOLDEN, "reference")
WATER = os.path.join(GOLDEN, "CornellBox", "CornellBox-Water")

SIZE_LIMIT = 845 * 1024       # no fixture larger than the largest one committed before (teapot.obj)
TOTAL_LIMIT = 1024 * 1024     # the whole directory: well under tests/golden's 1.4 MB before it

# ---- frame cases ------------------------------------------------------------------------------------
SHADERS = (0, 1, 3, 4)        # NoShadows, Whitted, DepthMap, DiffuseMaterial
ACCELERATORS = (0, 1, 2, 3)
OTHER_SIZES = ((30, 30), (96, 48), (128, 96))
UNSTABLE_EXPECTED = ((0, 1, 3, 100, 60),)


def frame_cases():
    """(scene, shader, accelerator, width, height) of every frame that must be a stable fixture."""
    out = [(sc, sh, a, 64, 64) for sc in (0, 1, 3) for sh in SHADERS for a in ACCELERATORS]
    out += [(2, sh, a, 64, 64) for sh in (3, 4) for a in ACCELERATORS]  # area lights: no light is sampled
    out += [(sc, 1, 3, w, h) for sc in (0, 3) for (w, h) in OTHER_SIZES]
    return out


def frame_name(case):
    return "s%d_sh%d_a%d_%dx%d" % tuple(case)


# ---- files ------------------------------------------------------------------------------------------
def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.dtype.str.encode() + repr(a.shape).encode() + a.tobytes()).hexdigest()


def save_npz(path, arrays):
    """A deflated .npz whose bytes depend on the arrays alone (fixed member order and timestamps)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def load(name):
    with np.load(os.path.join(FIXTURES, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def manifest():
    with open(os.path.join(FIXTURES, "manifest.json")) as f:
        return json.load(f)


def write_records(path, arrays):
    """ref_driver's file format: per array an int32 count of 4-byte words, then the words."""
    with open(path, "wb") as f:
        for a in arrays:
            a = np.ascontiguousarray(a)
            assert a.dtype.itemsize == 4, a.dtype
            f.write(np.int32(a.size).tobytes())
            f.write(a.tobytes())


def read_records(path):
    b = open(path, "rb").read()
    out, i = [], 0
    while i < len(b):
        n = int(np.frombuffer(b, np.int32, 1, i)[0])
        out.append(np.frombuffer(b, np.int32, n, i + 4).copy())
        i += 4 + 4 * n
    return out


def bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


# ---- meshes -----------------------------------------------------------------------------------------
MESHES = ("water", "degenerate")
MESH_W = MESH_H = 64
N_RAYS = 4096


def mesh_config(name, tmp, **kw):
    """mobileraytracer_amd.Config of a mesh case; `tmp`: a directory for the generated scene."""
    import mobileraytracer_amd as m
    if name == "water":
        obj, mtl, cam = (WATER + e for e in (".obj", ".mtl", ".cam"))
    else:
        import shape_scenes
        obj, mtl, cam, _ = shape_scenes.write_degenerate(str(tmp))
    kw.setdefault("width", MESH_W)
    kw.setdefault("height", MESH_H)
    return m.Config(sceneIndex=4, objFilePath=obj, mtlFilePath=mtl, camFilePath=cam, **kw)


def read_cam(path, ratio):
    """A perspective .cam file as the camera tuple (kind, position, lookAt, up, hFov, vFov) that the
    reference's loader hands to Perspective: the position's x negated (0 becomes -0), the horizontal
    field of view the file's times the aspect ratio, in float32."""
    v = {}
    for line in open(path):
        t = line.split()
        if t:
            v[t[0]] = t[1:]
    assert v["t"] == ["perspective"]
    p, l, u = (tuple(float(x) for x in v[k]) for k in "plu")
    p = (-p[0], p[1], p[2])
    return (0, p, l, u, float(F(float(v["f"][0])) * F(ratio)), float(F(float(v["f"][1]))))


def camera_row(cam):
    """A camera tuple as ref_driver's 12 floats."""
    kind, p, l, u, a, b = cam
    return np.array([kind, *p, *l, *u, a, b], F)


def _third_point(a, e):
    """B with B - A == e in float32, for the reference's builder, which takes points and subtracts."""
    b = a + e
    for _ in range(4):
        bad = (b - a) != e
        if not bad.any():
            return b
        b = np.where(bad & ((b - a) < e), np.nextafter(b, F(np.inf)), np.where(bad, np.nextafter(b, F(-np.inf)), b))
    raise AssertionError("an edge is not the difference of two float32 points")


def mesh_geometry(cfg):
    """What the reference's Scene is built from, out of the host-side scene accessors: triangle points
    (T, 9), materials (T,), material coefficients (M, 13), light kinds, light points (L, 9), light
    coefficients (L, 13).  No triangle of a mesh case has texture coordinates or a texture."""
    import mobileraytracer_amd as m
    geom, _, tex, mat = m.scene_triangles(cfg)
    coeffs, texture = m.scene_materials(cfg)
    lkind, lgeom, lcoeffs = m.scene_lights(cfg)
    assert (tex == -1).all() and (texture == -1).all()

    def points(g):
        a = g[:, 0]
        return np.concatenate([a, _third_point(a, g[:, 1]), _third_point(a, g[:, 2])], 1).astype(F)
    return [points(geom), mat.astype(np.int32), coeffs.astype(F), lkind.astype(np.int32),
            points(lgeom) if len(lgeom) else np.zeros((0, 9), F), lcoeffs.astype(F)]


def mesh_rays(points, seed):
    """N_RAYS rays for a mesh: half random from inside the scene's box, a quarter with one direction
    component zero, a quarter starting on a triangle and leaving along its plane; a random occlusion
    distance per ray."""
    rng = np.random.RandomState(seed)
    p = points.reshape(-1, 3, 3)
    lo, hi = p.min((0, 1)), p.max((0, 1))
    n = N_RAYS
    orig = (lo + rng.random_sample((n, 3)) * (hi - lo)).astype(F)
    dirs = rng.standard_normal((n, 3))
    q = n // 4
    dirs[2 * q:3 * q][np.arange(q), rng.randint(0, 3, q)] = 0.0
    a, ab, ac = p[:, 0].astype(np.float64), (p[:, 1] - p[:, 0]).astype(np.float64), (p[:, 2] - p[:, 0]).astype(np.float64)
    real = np.flatnonzero(np.linalg.norm(np.cross(ab, ac), axis=1) > 1e-6)
    t = real[rng.randint(0, len(real), q)]
    u = rng.random_sample(q)
    v = rng.random_sample(q) * (1 - u)
    orig[3 * q:] = (a[t] + u[:, None] * ab[t] + v[:, None] * ac[t]).astype(F)
    dirs[3 * q:] = rng.standard_normal((q, 1)) * ab[t] + rng.standard_normal((q, 1)) * ac[t]
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(F)
    dist = (rng.random_sample(n) * np.linalg.norm(hi - lo)).astype(F)
    assert np.isfinite(orig).all() and np.isfinite(dirs).all() and (np.abs(dirs).max(1) > 0).all()
    return orig, dirs, dist


# ---- cameras ----------------------------------------------------------------------------------------
CAMERA_SIZES = ((64, 48), (32, 16), (30, 30))
CAMERA_NAMES = ("scene0", "scene1", "scene2", "scene3", "water", "views0", "views1")


def cameras(w, h):
    """Per name of CAMERA_NAMES: (ref_driver's row, the product's camera tuple or None for the built-in
    camera of scene k).  The ratio is the frame's, as the reference computes it."""
    from test_views_gpu import CAMS
    ratio = F(w) / F(h)
    out = []
    for k in range(4):
        out.append((np.array([10 + k] + [0] * 9 + [ratio, 0], F), None))
    for cam in (read_cam(WATER + ".cam", ratio), CAMS[0], CAMS[1]):
        out.append((camera_row(cam), cam))
    return out


# the Constant pixel sampler's values per size: 0.5 no deviation, 1.0 and 0.0 plus and minus half a pixel.
# The deviations are recorded at 32 x 16, where deviationU != deviationV and every pixel is reached, and
# at 30 x 30; 64 x 48 has the undeviated rays only (the fixtures' bytes are nearly all camera directions).
CAMERA_DEVS = {(64, 48): (0.5,), (32, 16): (0.5, 1.0, 0.0), (30, 30): (0.5, 1.0, 0.0)}


def reached_pixels(w, h):
    """How many pixels the reference's 16 x 16 tiles of (w / 16) x (h / 16) pixels reach."""
    return 256 * (w // 16) * (h // 16)


def camera_rows(w, h):
    """(u, v, deviationU, deviationV) of every pixel, row-major, once per value of CAMERA_DEVS[w, h],
    as Renderer::renderScene computes them from a Constant sampler's value."""
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    u = (x.ravel().astype(F) * (F(1) / F(w))).astype(F)
    v = (y.ravel().astype(F) * (F(1) / F(h))).astype(F)
    rows = []
    for s in CAMERA_DEVS[w, h]:
        du = (F(s) - F(0.5)) * F(2) * (F(0.5) / F(w))
        dv = (F(s) - F(0.5)) * F(2) * (F(0.5) / F(h))
        # a deviated row of a frame that is not square tells deviationU from deviationV
        assert (du == dv) == (s == 0.5 or w == h)
        rows.append(np.stack([u, v, np.full_like(u, du), np.full_like(v, dv)], 1))
    return np.concatenate(rows).astype(F)


# ---- known-answer cases -----------------------------------------------------------------------------
def _ulps(x, k):
    x = np.asarray(x, F).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf))
    return x


def kat_inputs():
    """Triangle cases (n, 15: A B C origin direction), plane cases (n, 12: point normal origin
    direction), sphere cases (n, 10: centre radius origin direction), box cases (n, 12: min max origin
    direction)."""
    from test_device_kat import TRI_CASES
    from test_oracle_kat import TRI, sub
    rng = np.random.RandomState(20240611)
    n, e = 4096, 512
    # triangles: the reference's unit-test vectors, random pairs aimed at the triangle's neighbourhood,
    # and rays aimed within +-2 ulp (per coordinate) of a point on an edge or of a vertex
    first = np.array([np.concatenate([np.ravel(TRI), c[0], sub(c[1], c[0])]) for c in TRI_CASES], F)
    abc = (rng.standard_normal((n + e, 3, 3)) * 2).astype(F)
    orig = (rng.standard_normal((n + e, 3)) * 4).astype(F)
    w = rng.random_sample((n + e, 3)) * 1.6 - 0.3           # barycentric, some outside
    w /= w.sum(1, keepdims=True)
    target = np.einsum("nk,nkc->nc", w[:n], abc[:n].astype(np.float64)).astype(F)
    where = rng.randint(0, 6, e)                            # 0-2: vertex, 3-5: on the edge from that vertex
    s = rng.random_sample(e)
    va, vb = abc[n:][np.arange(e), where % 3], abc[n:][np.arange(e), (where + 1) % 3]
    on = np.where((where >= 3)[:, None], (va + s[:, None].astype(F) * (vb - va)).astype(F), va).astype(F)
    k = rng.randint(-2, 3, (e, 3))
    near = on.copy()
    for d in (-2, -1, 1, 2):
        near = np.where(k == d, _ulps(on, d), near)
    target = np.concatenate([target, near])
    tri = np.concatenate([first, np.concatenate([abc.reshape(-1, 9), orig, (target - orig).astype(F)], 1)]).astype(F)
    # planes
    normal = rng.standard_normal((n, 3))
    normal = (normal / np.linalg.norm(normal, axis=1, keepdims=True)).astype(F)
    plane = np.concatenate([(rng.standard_normal((n, 3)) * 2).astype(F), normal, (rng.standard_normal((n, 3)) * 4).astype(F),
                            rng.standard_normal((n, 3)).astype(F)], 1).astype(F)
    plane[::16, 9:] = np.cross(plane[::16, 3:6], rng.standard_normal((n // 16, 3))).astype(F)  # (nearly) parallel
    # spheres: rays aimed near the sphere, some from inside
    centre = (rng.standard_normal((n, 3)) * 2).astype(F)
    radius = (rng.random_sample((n, 1)) * 1.5 + 0.05).astype(F)
    so = (centre + rng.standard_normal((n, 3)) * radius * np.where(rng.random_sample((n, 1)) < 0.2, 0.5, 4.0)).astype(F)
    aim = centre + rng.standard_normal((n, 3)) * radius * 0.8
    sphere = np.concatenate([centre, radius, so, (aim - so).astype(F)], 1).astype(F)
    # boxes: the unit-test vectors (zero-thickness boxes, NaN paths), random ones, flat axes and
    # origins on a face
    kat = [((0, 0, 0), (1, 0, 0), (2, 0, 0), (-1, 0, 0)), ((0, 0, 0), (1, 0, 0), (2, 0, 0), (1, 0, 0)),
           ((0, 0, 0), (0, 1, 1), (0, 0.5, 2), (0, 0, -1)), ((0, 0, 0), (1, 1, 1), (0.5, 0.5, -3), (0, 0, 1))]
    m = n + e
    lo = rng.standard_normal((m, 3)).astype(F)
    ext = np.abs(rng.standard_normal((m, 3))).astype(F)
    bo = (rng.standard_normal((m, 3)) * 3).astype(F)
    bd = ((lo + ext * (rng.random_sample((m, 3)) * 1.6 - 0.3)).astype(F) - bo).astype(F)  # aimed at the box's neighbourhood
    axis = rng.randint(0, 3, e)
    flat = rng.random_sample(e) < 0.5
    ext[n:][np.arange(e)[flat], axis[flat]] = 0
    hi = (lo + ext).astype(F)
    face = ~flat
    bo[n:][np.arange(e)[face], axis[face]] = np.where(rng.random_sample(face.sum()) < 0.5, lo[n:][np.arange(e)[face], axis[face]],
                                                      hi[n:][np.arange(e)[face], axis[face]])
    zero = rng.random_sample(e) < 0.5
    bd[n:][np.arange(e)[zero], rng.randint(0, 3, e)[zero]] = 0
    box = np.concatenate([np.array([np.concatenate(c) for c in kat], F), np.concatenate([lo, hi, bo, bd], 1)]).astype(F)
    return tri, plane, sphere, box


# ---- pixel conversion -------------------------------------------------------------------------------
AVG_N = (1, 2, 3, 8, 255)


def avg_inputs():
    """(rgb (R, 3), previous average (R,) int32, n (R,) int32): tests/test_accumulate_kat.py's value
    table in each channel (the other two ordinary) over a set of previous averages, at every n of AVG_N."""
    from test_accumulate_kat import TABLE
    rng = np.random.RandomState(11)
    prior = np.array([0, 0x00808080, 0xFFFFFFFF] + [int(x) for x in rng.randint(0, 1 << 32, 5, np.int64)], np.uint32)
    rgb, avg, num = [], [], []
    for n in AVG_N:
        for c in range(3):
            for x in TABLE:
                for a in prior:
                    row = rng.random_sample(3).astype(F)
                    row[c] = x
                    rgb.append(row)
                    avg.append(a)
                    num.append(n)
    return np.array(rgb, F), np.array(avg, np.uint32).view(np.int32), np.array(num, np.int32)
