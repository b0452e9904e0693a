"""What a nearest-point query costs: nearest_points_device on 2^20 points on the Conference stand-in, with
cast_rays_device on 2^20 rays (the incoherent set of tools/ray_query_bench.py) beside it for scale.

Two point distributions:
  uniform  points uniform in the scene's bounding box;
  surface  random surface points (a uniform triangle, uniform barycentrics) moved by up to 1 % of the box
           diagonal per axis.

One process and one renderer (2048 x 2048, Whitted: a level-1 queue of 2^22 rays, one chunk per call);
everything resident beforehand, events on the caller's stream around each call, the three arms
alternating; median and range of --reps rounds after --warmup warm-up rounds.  Beside the times the mean
of `tests` per point (distance-function evaluations: a walk that never culls makes one per triangle).

  python tools/nearest_bench.py [--reps 20] [--warmup 3] [--out profiles/nearest_bench.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mobileraytracer_amd as m  # noqa: E402
from ray_query_bench import config, incoherent  # noqa: E402

N = 1 << 20


def uniform_points(n, lo, hi, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (lo + torch.rand((n, 3), device="cuda", generator=g) * (hi - lo)).contiguous()


def surface_points(n, geom, diag, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = geom[torch.randint(0, len(geom), (n,), device="cuda", generator=g)]
    w = torch.rand((n, 2), device="cuda", generator=g)
    flip = w.sum(1) > 1
    w[flip] = 1 - w[flip]
    p = t[:, 0] + w[:, :1] * t[:, 1] + w[:, 1:] * t[:, 2]
    return (p + (torch.rand((n, 3), device="cuda", generator=g) * 2 - 1) * (0.01 * diag)).contiguous()


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
    emit("# python tools/nearest_bench.py " + " ".join(sys.argv[1:]))
    emit("# nearest_points_device and cast_rays_device, n = 2^20 each, events on the caller's stream, one process,")
    emit("# the arms alternating; median [least .. largest] of %d rounds after %d warm-up rounds" % (a.reps, a.warmup))
    cfg = config()
    boxes = m.triangle_bvh(cfg)[0]
    lo, hi = torch.from_numpy(boxes[0, :3].copy()).cuda(), torch.from_numpy(boxes[0, 3:].copy()).cuda()
    diag = float(torch.linalg.norm(hi - lo))
    geom = torch.from_numpy(m.scene_triangles(cfg)[0]).cuda()
    stream = torch.cuda.Stream()
    sets = {"uniform": uniform_points(N, lo, hi, 3), "surface": surface_points(N, geom, diag, 4)}
    o, d = incoherent(N, lo, hi, 7)
    kind = torch.empty(N, dtype=torch.int32, device="cuda")
    index = torch.empty(N, dtype=torch.int32, device="cuda")
    t = torch.empty(N, dtype=torch.float32, device="cuda")
    point = torch.empty((N, 3), dtype=torch.float32, device="cuda")
    bary = torch.empty((N, 2), dtype=torch.float32, device="cuda")
    tests = torch.empty(N, dtype=torch.int32, device="cuda")
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

        def nearest_arm(pts):
            return lambda: r.nearest_points_device(pts.data_ptr(), N, d_kind=kind.data_ptr(), d_index=index.data_ptr(),
                                                   d_dist2=t.data_ptr(), d_point=point.data_ptr(), d_bary=bary.data_ptr(),
                                                   d_tests=tests.data_ptr(), stream=stream.cuda_stream)

        arms = [("nearest_points_device, " + name, nearest_arm(pts)) for name, pts in sets.items()]
        arms.append(("cast_rays_device, incoherent", lambda: r.cast_rays_device(
            o.data_ptr(), d.data_ptr(), N, d_kind=kind.data_ptr(), d_index=index.data_ptr(), d_t=t.data_ptr(),
            stream=stream.cuda_stream)))
        means = {}
        for name, call in arms[:2]:  # (also the first warm-up round)
            timed(call)
            found = float((kind > 0).float().mean())
            means[name] = (float(tests.float().mean()), found, float(t.sqrt().mean()) / diag)
        for _ in range(a.warmup):
            for _, call in arms:
                timed(call)
        ms = {name: [] for name, _ in arms}
        for _ in range(a.reps):
            for name, call in arms:
                ms[name].append(timed(call))
        for name, _ in arms:
            x = ms[name]
            extra = ""
            if name in means:
                extra = "   mean tests per point %8.1f   found %5.1f %%   mean distance %.4f diagonals" % (
                    means[name][0], 100.0 * means[name][1], means[name][2])
            emit("%-34s %8.3f ms [%8.3f .. %8.3f]   %7.1f M / s%s" % (name, statistics.median(x), min(x), max(x),
                                                                     N / statistics.median(x) * 1e-3, extra))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
