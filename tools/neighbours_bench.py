"""What a neighbour query costs: neighbours_device on 2^20 points on the Conference stand-in, with
nearest_points_device on the same points beside it.

Arms, on the `surface` points of tools/nearest_bench.py (random surface points moved by up to 1 % of the
box diagonal per axis):
  nearest_points_device                       every field
  neighbours_device, K = 1 / 4 / 16           every field but count: the K-nearest search
  neighbours_device, K = 16, count, radius    every field, a radius of 1 % of the box diagonal: every surface
                                              within the radius is met

One process and one renderer (2048 x 2048, Whitted: a level-1 queue of 2^22 rays, one chunk per call);
everything resident beforehand, events on the caller's stream around each call, the arms alternating;
median and range of --reps rounds after --warmup warm-up rounds.  Beside the times the mean of `tests` per
point (distance-function evaluations) and, for the counted arm, the mean count.

  python tools/neighbours_bench.py [--reps 20] [--warmup 3] [--out profiles/neighbours_bench.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import mobileraytracer_amd as m  # noqa: E402
from nearest_bench import surface_points  # noqa: E402
from ray_query_bench import config  # noqa: E402

N = 1 << 20
K_MAX = 16


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--out", default="")
    a = p.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit("# python tools/neighbours_bench.py " + " ".join(sys.argv[1:]))
    emit("# nearest_points_device and neighbours_device, n = 2^20 surface points, events on the caller's stream, one")
    emit("# process, the arms alternating; median [least .. largest] of %d rounds after %d warm-up rounds" % (a.reps, a.warmup))
    cfg = config()
    boxes = m.triangle_bvh(cfg)[0]
    lo, hi = torch.from_numpy(boxes[0, :3].copy()).cuda(), torch.from_numpy(boxes[0, 3:].copy()).cuda()
    diag = float(torch.linalg.norm(hi - lo))
    geom = torch.from_numpy(m.scene_triangles(cfg)[0]).cuda()
    stream = torch.cuda.Stream()
    pts = surface_points(N, geom, diag, 4)
    radius = torch.full((N,), 0.01 * diag, dtype=torch.float32, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    f32 = dict(dtype=torch.float32, device="cuda")
    out = {"count": torch.empty(N, **i32), "kind": torch.empty(N * K_MAX, **i32), "index": torch.empty(N * K_MAX, **i32),
           "dist2": torch.empty(N * K_MAX, **f32), "point": torch.empty(N * K_MAX * 3, **f32),
           "bary": torch.empty(N * K_MAX * 2, **f32), "tests": torch.empty(N, **i32)}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with m.Renderer(cfg) as r:
        q, info = r.queue_info(), r.scene_info()
        emit("# Conference stand-in, %d triangles, box diagonal %.2f; renderer 2048 x 2048 Whitted: level-1 queue %d rays"
             % (info["triangles"], diag, q["rayCap"][0]))

        def timed(call):
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        def nearest_arm():
            r.nearest_points_device(pts.data_ptr(), N, stream=stream.cuda_stream,
                                    **{"d_" + f: x.data_ptr() for f, x in out.items() if f != "count"})

        def neighbour_arm(k, counted):
            ptrs = {"d_" + f: x.data_ptr() for f, x in out.items() if counted or f != "count"}
            return lambda: r.neighbours_device(pts.data_ptr(), N, k, d_dist=radius.data_ptr() if counted else 0,
                                               stream=stream.cuda_stream, **ptrs)

        arms = [("nearest_points_device", nearest_arm)]
        arms += [("neighbours_device, K = %d" % k, neighbour_arm(k, False)) for k in (1, 4, K_MAX)]
        arms.append(("neighbours_device, K = %d, count, radius 1 %%" % K_MAX, neighbour_arm(K_MAX, True)))
        notes = {}
        for name, call in arms:  # (also the first warm-up round)
            out["count"].fill_(-1)
            torch.cuda.synchronize()
            timed(call)
            notes[name] = "   mean tests per point %8.1f" % float(out["tests"].float().mean())
            if name.endswith("%"):
                notes[name] += "   mean count %.1f, largest %d" % (float(out["count"].float().mean()), int(out["count"].max()))
        for _ in range(a.warmup):
            for _, call in arms:
                timed(call)
        ms = {name: [] for name, _ in arms}
        for _ in range(a.reps):
            for name, call in arms:
                ms[name].append(timed(call))
        for name, _ in arms:
            x = ms[name]
            emit("%-44s %8.3f ms [%8.3f .. %8.3f]   %7.1f M / s%s" % (name, statistics.median(x), min(x), max(x),
                                                                     N / statistics.median(x) * 1e-3, notes[name]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
