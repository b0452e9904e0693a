"""Records tests/golden/reference/: what the reference's own code returns on the cases of
tests/reference_cases.py.  Run after ``__graft_entry__.build()`` has built oracle/_ref/ref_driver
(oracle/ref_build.py; it needs a reference tree):

    python tests/golden/make_reference_fixtures.py

A frame is recorded only if three fresh processes, each of which reseeds the reference's tile order
and sample tables from std::random_device, return the same bytes; a frame that does not is listed in
the manifest under "unstable" with the number of pixels that differed, and is no fixture.  Apart from
the manifest's compiler line and an unstable case's pixel count, a second run writes the same bytes.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import reference_cases as C  # noqa: E402
from oracle import ref_build  # noqa: E402

RUNS = 3


def driver(*args):
    subprocess.run([ref_build.DRIVER] + [str(a) for a in args], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)


def count(words):
    return np.array([int(np.uint32(words[0])) | (int(np.uint32(words[1])) << 32)], np.int64)


def stable(run):
    """`run()` in RUNS fresh processes: (records of the first, per record the largest number of words
    in which a later run differed from it)."""
    first = run()
    differ = [0] * len(first)
    for _ in range(RUNS - 1):
        again = run()
        differ = [max(d, int((a != b).sum())) for d, a, b in zip(differ, first, again)]
    return first, differ


def record_frames(tmp, man):
    out = os.path.join(tmp, "frame.bin")
    arrays = {}
    for case in C.frame_cases() + list(C.UNSTABLE_EXPECTED):
        def run():
            driver("frame", *case, out)
            return C.read_records(out)
        (bitmap, rays), differ = stable(run)
        name = C.frame_name(case)
        if any(differ):
            man["unstable"].append({"case": name, "args": list(case), "pixelsDiffering": differ[0], "runs": RUNS})
            print("unstable: %s, %d pixels differ between runs" % (name, differ[0]))
            continue
        arrays[name] = bitmap
        arrays[name + "_rays"] = count(rays)
        man["cases"][name] = {"mode": "frame", "args": list(case), "file": "frames.npz",
                              "outputs": {name: C.sha(bitmap), name + "_rays": C.sha(arrays[name + "_rays"])}}
    C.save_npz(os.path.join(C.FIXTURES, "frames.npz"), arrays)


def record_mesh(tmp, man, name, seed):
    import mobileraytracer_amd as m  # noqa: F401  (the host-side scene accessors; no GPU)
    cfg = C.mesh_config(name, os.path.join(tmp, name))
    geometry = C.mesh_geometry(cfg)
    camera = C.camera_row(C.read_cam(cfg.camFilePath, np.float32(C.MESH_W) / np.float32(C.MESH_H)))
    bound = np.array([1, 1, 1], np.float32)  # the reference's DepthMap bound for a loaded scene
    orig, dirs, dist = C.mesh_rays(geometry[0], seed)
    fin, fout = os.path.join(tmp, name + ".in"), os.path.join(tmp, name + ".out")
    C.write_records(fin, geometry + [camera, bound, orig, dirs, dist])

    def run():
        driver("mesh", fin, fout, C.MESH_W, C.MESH_H)
        return C.read_records(fout)
    recs, differ = stable(run)
    assert len(recs) == 3 * 8 + 2
    arrays = {"orig": orig, "dirs": dirs, "dist": dist, "camera": camera, "bound": bound}
    inputs = {k: C.sha(v) for k, v in arrays.items()}
    inputs.update({"geometry%d" % i: C.sha(g) for i, g in enumerate(geometry)})
    outputs = {}
    fields = ("kind", "index", "t", "occluded", "depth", "depth_rays", "diffuse", "diffuse_rays")
    for a in (1, 2, 3):
        for f, r, d in zip(fields, recs[8 * (a - 1):8 * a], differ[8 * (a - 1):8 * a]):
            key = "a%d_%s" % (a, f)
            if d:
                man["unstable"].append({"case": "mesh_%s/%s" % (name, key), "pixelsDiffering": d, "runs": RUNS})
                print("unstable: mesh_%s/%s, %d words differ between runs" % (name, key, d))
                continue
            outputs[key] = count(r) if f.endswith("_rays") else r
    outputs["bvh_order"], outputs["grid_order"] = recs[24], recs[25]
    assert not differ[24] and not differ[25]
    arrays.update(outputs)
    C.save_npz(os.path.join(C.FIXTURES, "mesh_%s.npz" % name), arrays)
    man["cases"]["mesh_" + name] = {"mode": "mesh", "args": [name, C.MESH_W, C.MESH_H, seed], "file": "mesh_%s.npz" % name,
                                    "triangles": int(len(geometry[1])), "lights": int(len(geometry[3])),
                                    "inputs": inputs, "outputs": {k: C.sha(v) for k, v in outputs.items()}}


def record_cameras(tmp, man):
    fin, fout = os.path.join(tmp, "cam.in"), os.path.join(tmp, "cam.out")
    arrays = {}
    for (w, h) in C.CAMERA_SIZES:
        cams, rows = C.cameras(w, h), C.camera_rows(w, h)
        C.write_records(fin, [np.concatenate([c[0] for c in cams]), rows])
        driver("camera", fin, fout)
        recs = C.read_records(fout)
        for k, name in enumerate(C.CAMERA_NAMES):
            key = "%s_%dx%d" % (name, w, h)
            if name == "scene2":  # the reference pairs scene 2 with scene 0's camera: stored once
                assert np.array_equal(recs[2 * k], recs[0]) and np.array_equal(recs[2 * k + 1], recs[1])
                key = "scene0_%dx%d" % (w, h)
            arrays[key + "_orig"] = recs[2 * k].reshape(-1, 3)
            arrays[key + "_dirs"] = recs[2 * k + 1].reshape(-1, 3)
            man["cases"]["camera_%s_%dx%d" % (name, w, h)] = {
                "mode": "camera", "args": [name, w, h], "file": "cameras.npz",
                "inputs": {"camera": C.sha(cams[k][0]), "rows": C.sha(rows)},
                "outputs": {key + "_orig": C.sha(arrays[key + "_orig"]), key + "_dirs": C.sha(arrays[key + "_dirs"])}}
    C.save_npz(os.path.join(C.FIXTURES, "cameras.npz"), arrays)


def record_kat(tmp, man):
    fin, fout = os.path.join(tmp, "kat.in"), os.path.join(tmp, "kat.out")
    inputs = C.kat_inputs()
    C.write_records(fin, inputs)
    driver("kat", fin, fout)
    names = ("triangle_hit", "triangle_t", "plane_hit", "plane_t", "sphere_hit", "sphere_t", "box_hit")
    arrays = dict(zip(names, C.read_records(fout)))
    C.save_npz(os.path.join(C.FIXTURES, "kat.npz"), arrays)
    man["cases"]["kat"] = {"mode": "kat", "args": [len(x) for x in inputs], "file": "kat.npz",
                           "inputs": {k: C.sha(v) for k, v in zip(("triangle", "plane", "sphere", "box"), inputs)},
                           "outputs": {k: C.sha(v) for k, v in arrays.items()}}


def record_avg(tmp, man):
    fin, fout = os.path.join(tmp, "avg.in"), os.path.join(tmp, "avg.out")
    inputs = C.avg_inputs()
    C.write_records(fin, inputs)
    driver("avg", fin, fout)
    arrays = {"result": C.read_records(fout)[0]}
    C.save_npz(os.path.join(C.FIXTURES, "avg.npz"), arrays)
    man["cases"]["avg"] = {"mode": "avg", "args": list(C.AVG_N), "file": "avg.npz",
                           "inputs": {k: C.sha(v) for k, v in zip(("rgb", "average", "n"), inputs)},
                           "outputs": {"result": C.sha(arrays["result"])}}


def main():
    if not ref_build.build():
        sys.exit("make_reference_fixtures: oracle/_ref/ref_driver is not built (no reference tree?)")
    os.makedirs(C.FIXTURES, exist_ok=True)
    man = {"compiler": ref_build.compiler_version(), "flags": ref_build.FLAGS, "runs": RUNS, "cases": {}, "unstable": []}
    with tempfile.TemporaryDirectory() as tmp:
        record_frames(tmp, man)
        for k, name in enumerate(C.MESHES):
            record_mesh(tmp, man, name, 7001 + k)
        record_cameras(tmp, man)
        record_kat(tmp, man)
        record_avg(tmp, man)
    with open(os.path.join(C.FIXTURES, "manifest.json"), "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)
        f.write("\n")
    sizes = {n: os.path.getsize(os.path.join(C.FIXTURES, n)) for n in sorted(os.listdir(C.FIXTURES))}
    print("recorded %d cases, %d unstable; bytes: %s, total %d" % (len(man["cases"]), len(man["unstable"]), sizes,
                                                                     sum(sizes.values())))


if __name__ == "__main__":
    main()
