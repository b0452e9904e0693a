"""Scenes whose content decides which code runs after the walk (tests only).

* ``write_extreme``: the glassboxes fixture with ONE line of its MTL replaced - a non-finite, huge or
  negative coefficient.  These reach the float -> pixel conversion outside [0, 2^32) and the
  ``matsFinite`` flag of the depth-capped level (DESIGN.md sections 2 and 4).
* ``write_table_scene``: M ordinary materials and Q emissive quads, to put the lean ``k_shade``'s
  LDS table of materials and lights below, at and above its 64 records.
"""
import os
import shutil

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glassboxes")

# name -> (material, key, replacement line); None: the unchanged twin
EXTREME = {
    "kd_inf": ("glass", "Kd", "Kd 1e39 0.2 0.2"),       # parses to inf: Kd * 0 = NaN at the depth cap
    "ks_inf": ("glass", "Ks", "Ks 1e39 0.3 0.3"),
    "kt_inf": ("glass", "Tf", "Tf 1e39 0.6 0.6"),       # Kt = Tf * (1 - d) = inf
    "kd_huge": ("glass", "Kd", "Kd 3e38 0.2 0.2"),      # finite; overflows in flight
    "kd_neg": ("glass", "Kd", "Kd -0.5 0.2 0.2"),       # negative radiance: the uint32 wrap
    "ke_neg": ("light", "Ke", "Ke 10 -10 10"),
    "ke_inf": ("light", "Ke", "Ke 1e39 1e39 1e39"),     # normalised to NaN: no longer emissive
    "plain": None,
}
NON_FINITE = ("kd_inf", "ks_inf", "kt_inf")  # scenes whose Kd / Ks / Kt has a non-finite component


def write_extreme(path, name):
    """OBJ / MTL / CAM of the scene `name` in directory `path` (created)."""
    os.makedirs(path, exist_ok=True)
    obj, mtl, cam = (os.path.join(path, "glassboxes." + e) for e in ("obj", "mtl", "cam"))
    shutil.copyfile(os.path.join(GOLDEN, "glassboxes.obj"), obj)
    shutil.copyfile(os.path.join(GOLDEN, "glassboxes.cam"), cam)
    change = EXTREME[name]
    out, current, replaced = [], None, 0
    with open(os.path.join(GOLDEN, "glassboxes.mtl")) as f:
        for line in f:
            t = line.split()
            if t and t[0] == "newmtl":
                current = t[1]
            if change is not None and t and current == change[0] and t[0] == change[1]:
                line = "    " + change[2] + "\n"
                replaced += 1
            out.append(line)
    assert replaced == (0 if change is None else 1), (name, replaced)
    with open(mtl, "w") as f:
        f.writelines(out)
    return obj, mtl, cam


# ---- many materials, many lights ----------------------------------------------------------------
def _q(x):  # snap to the 1/64 grid: exact in float32 and as short decimal text for every parser
    return round(x * 64.0) / 64.0


def material_kd(i):
    """Material i's Kd: three multiples of 1/64 in (0, 1), distinct for every i < 63 * 63."""
    return (1 + i % 63) / 64.0, (1 + (i // 63) % 63) / 64.0, (1 + (7 * i) % 63) / 64.0


def table_records(materials, lights):
    """float4 records of the lean k_shade's LDS table, as launchShade counts them: 4 per material,
    then 4 per light (the launch takes the general kernel when this exceeds 256)."""
    return 4 * (materials + lights)


def write_table_scene(path, n_mats, n_quads):
    """A floor, a back wall, a grid of `n_mats` small camera-facing quads each with its own material,
    and `n_quads` emissive quads overhead (two triangles, so two lights, each).  The scene then has
    n_mats + 2 materials and 2 * n_quads lights.  Returns (obj, mtl, cam)."""
    os.makedirs(path, exist_ok=True)
    obj, mtl, cam = (os.path.join(path, "tables." + e) for e in ("obj", "mtl", "cam"))
    verts, faces = [], []  # faces: (material name, 4 vertex indices)

    def quad(name, a, b, c, d):
        k = len(verts)
        verts.extend([a, b, c, d])
        faces.append((name, (k + 4, k + 3, k + 2, k + 1)))

    with open(mtl, "w") as f:
        f.write("newmtl floor\nKd 0.75 0.75 0.75\nKs 0 0 0\n\n")
        f.write("newmtl wall\nKd 0.5 0.25 0.75\nKs 0 0 0\n\n")
        for i in range(n_mats):
            f.write("newmtl m%d\nKd %r %r %r\n" % ((i,) + material_kd(i)))
            f.write("Ks 0.25 0.25 0.25\n" if i % 8 == 0 else "Ks 0 0 0\n")
            if i % 16 == 0:
                f.write("Tf 0.6 0.6 0.6\nd 0.5\nNi 1.5\n")
            f.write("\n")
        f.write("newmtl light\nKd 0.78 0.78 0.78\nKs 0 0 0\nKe 10 10 10\n")
    quad("floor", (-8, -5, -10), (8, -5, -10), (8, -5, 3), (-8, -5, 3))
    quad("wall", (-8, -5, 2), (8, -5, 2), (8, 6, 2), (-8, 6, 2))
    cols = 1
    while cols * cols < n_mats:
        cols += 1
    cell = _q(8.0 / cols - 1.0 / 128.0)  # rounded down to the grid: the whole grid inside [-4, 4]
    size = max(_q(0.75 * cell), 1.0 / 64.0)
    for i in range(n_mats):
        x0, y0 = -4.0 + (i % cols) * cell, -4.0 + (i // cols) * cell
        z = _q(-(i % 5) / 8.0)  # five depths, so neighbours shadow and reflect each other
        quad("m%d" % i, (x0, y0, z), (x0 + size, y0, z), (x0 + size, y0 + size, z), (x0, y0 + size, z))
    per_row = 5
    for k in range(n_quads):
        x0, z0 = -3.75 + 1.5 * (k % per_row), -7.0 + 1.5 * (k // per_row)
        quad("light", (x0, 5.5, z0), (x0 + 1.0, 5.5, z0), (x0 + 1.0, 5.5, z0 + 1.0), (x0, 5.5, z0 + 1.0))
    with open(obj, "w") as f:
        f.write("mtllib tables.mtl\n")
        for v in verts:
            f.write("v %r %r %r\n" % tuple(float(c) for c in v))
        last = None
        for name, idx in faces:
            if name != last:
                f.write("usemtl %s\n" % name)
                last = name
            f.write("f %d %d %d %d\n" % idx)
    with open(cam, "w") as f:
        f.write("t perspective\np 0 0 -10\nl 0 0 0\nu 0 1 0\nf 60 60\n")
    return obj, mtl, cam
