"""What a sweep query costs: sweep_spheres_device on 2^20 sweeps on the Conference stand-in, with
cast_rays_device and nearest_points_device on the same origins beside it.

The sweeps start at random surface points (a uniform triangle, uniform barycentrics) offset along the
triangle's normal by two radii, and move in random directions; the radius is 1 % of the box diagonal, the
direction has the length of one radius and the bound is 10, so a sweep covers at most 10 radii.  Arms:
  sweep_spheres_device, every field           the first contact, its centre, point and barycentrics
  sweep_spheres_device, hit only              "is this move free": the walk stops at a ray's first acceptance
  cast_rays_device                            the closest hit along the same rays (unit directions), unbounded
  nearest_points_device                       the nearest surface to the same origins, unbounded

One process and one renderer (2048 x 2048, Whitted: a level-1 queue of 2^22 rays, one chunk per call);
everything resident beforehand, events on the caller's stream around each call, the arms alternating;
median and range of --reps rounds after --warmup warm-up rounds.  Beside the times the mean of `tests` per
sweep (sweep- or distance-function evaluations) and the share of sweeps that hit.

  python tools/sweep_bench.py [--reps 20] [--warmup 3] [--out profiles/sweep_bench.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import mobileraytracer_amd as m  # noqa: E402
from ray_query_bench import config  # noqa: E402

N = 1 << 20


def sweeps(n, geom, radius, seed):
    """Origins two radii off random surface points along the normal, unit directions."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = geom[torch.randint(0, len(geom), (n,), device="cuda", generator=g)]
    w = torch.rand((n, 2), device="cuda", generator=g)
    flip = w.sum(1) > 1
    w[flip] = 1 - w[flip]
    p = t[:, 0] + w[:, :1] * t[:, 1] + w[:, 1:] * t[:, 2]
    nrm = torch.linalg.cross(t[:, 1], t[:, 2])
    nrm = nrm / torch.linalg.norm(nrm, dim=1, keepdim=True).clamp_min(1e-30)
    d = torch.randn((n, 3), device="cuda", generator=g)
    d = d / torch.linalg.norm(d, dim=1, keepdim=True)
    return (p + nrm * (2 * radius)).contiguous(), d.contiguous()


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
    emit("# python tools/sweep_bench.py " + " ".join(sys.argv[1:]))
    emit("# sweep_spheres_device, cast_rays_device and nearest_points_device, n = 2^20 each on the same origins, events on the")
    emit("# caller's stream, one process, the arms alternating; median [least .. largest] of %d rounds after %d warm-up rounds" % (
        a.reps, a.warmup))
    cfg = config()
    root = m.triangle_bvh(cfg)[0]
    lo, hi = torch.from_numpy(root[0, :3].copy()).cuda(), torch.from_numpy(root[0, 3:].copy()).cuda()
    diag = float(torch.linalg.norm(hi - lo))
    geom = torch.from_numpy(m.scene_triangles(cfg)[0]).cuda()
    stream = torch.cuda.Stream()
    rad = 0.01 * diag
    o, unit = sweeps(N, geom, rad, 5)
    d = (unit * rad).contiguous()  # t counts radii
    radius = torch.full((N,), rad, dtype=torch.float32, device="cuda")
    bound = torch.full((N,), 10.0, dtype=torch.float32, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    f32 = dict(dtype=torch.float32, device="cuda")
    out = {"hit": torch.empty(N, **i32), "kind": torch.empty(N, **i32), "index": torch.empty(N, **i32),
           "t": torch.empty(N, **f32), "centre": torch.empty(N * 3, **f32), "point": torch.empty(N * 3, **f32),
           "bary": torch.empty(N * 2, **f32), "tests": torch.empty(N, **i32)}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with m.Renderer(cfg) as r:
        q, info = r.queue_info(), r.scene_info()
        emit("# Conference stand-in, %d triangles, box diagonal %.2f, radius %.3f, at most 10 radii per sweep; renderer "
             "2048 x 2048 Whitted: level-1 queue %d rays" % (info["triangles"], diag, rad, q["rayCap"][0]))

        def timed(call):
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        def sweep_arm(fields):
            ptrs = {"d_" + f: out[f].data_ptr() for f in fields}
            return lambda: r.sweep_spheres_device(o.data_ptr(), d.data_ptr(), radius.data_ptr(), N, d_dist=bound.data_ptr(),
                                                  stream=stream.cuda_stream, **ptrs)

        def cast_arm():
            r.cast_rays_device(o.data_ptr(), unit.data_ptr(), N, d_kind=out["kind"].data_ptr(), d_index=out["index"].data_ptr(),
                               d_t=out["t"].data_ptr(), stream=stream.cuda_stream)

        def nearest_arm():
            r.nearest_points_device(o.data_ptr(), N, d_kind=out["kind"].data_ptr(), d_index=out["index"].data_ptr(),
                                    d_dist2=out["t"].data_ptr(), d_point=out["point"].data_ptr(), d_bary=out["bary"].data_ptr(),
                                    d_tests=out["tests"].data_ptr(), stream=stream.cuda_stream)

        arms = [("sweep_spheres_device, every field", sweep_arm(tuple(out)), "hit"),
                ("sweep_spheres_device, hit only", sweep_arm(("hit", "tests")), "hit"),
                ("cast_rays_device", cast_arm, ""),
                ("nearest_points_device", nearest_arm, "tests")]
        notes = {}
        for name, call, field in arms:  # (also the first warm-up round)
            out["tests"].fill_(0)
            out["hit"].fill_(0)
            torch.cuda.synchronize()
            timed(call)
            notes[name] = ""
            if field:
                notes[name] = "   mean tests per query %8.1f" % float(out["tests"].float().mean())
            if field == "hit":
                notes[name] += "   hit share %.3f" % float(out["hit"].float().mean())
        for _ in range(a.warmup):
            for _, call, _ in arms:
                timed(call)
        ms = {name: [] for name, _, _ in arms}
        for _ in range(a.reps):
            for name, call, _ in arms:
                ms[name].append(timed(call))
        for name, _, _ in arms:
            x = ms[name]
            emit("%-36s %8.3f ms [%8.3f .. %8.3f]   %7.1f M / s%s" % (name, statistics.median(x), min(x), max(x),
                                                                     N / statistics.median(x) * 1e-3, notes[name]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
