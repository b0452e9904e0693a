"""What an overlap query costs: overlap_boxes_device on 2^20 boxes on the Conference stand-in, with
neighbours_device on the boxes' centres beside it.

The boxes are cubes of half-side 1 % of the box diagonal, centred on the `surface` points of
tools/nearest_bench.py (random surface points moved by up to 1 % of the diagonal per axis).  Arms:
  overlap_boxes_device, any only              the occupancy test: the walk stops at a box's first acceptance
  overlap_boxes_device, count only            every accepted candidate met, no list
  overlap_boxes_device, K = 16, count         every field
  neighbours_device, K = 16, count, radius    every field, a radius equal to the half-side

One process and one renderer (2048 x 2048, Whitted: a level-1 queue of 2^22 rays, one chunk per call);
everything resident beforehand, events on the caller's stream around each call, the arms alternating;
median and range of --reps rounds after --warmup warm-up rounds.  Beside the times the mean of `tests` per
box (overlap- or distance-function evaluations) and the mean count.

  python tools/overlap_bench.py [--reps 20] [--warmup 3] [--out profiles/overlap_bench.txt]
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
    emit("# python tools/overlap_bench.py " + " ".join(sys.argv[1:]))
    emit("# overlap_boxes_device and neighbours_device, n = 2^20 cubes about surface points, events on the caller's stream,")
    emit("# one process, the arms alternating; median [least .. largest] of %d rounds after %d warm-up rounds" % (a.reps, a.warmup))
    cfg = config()
    root = m.triangle_bvh(cfg)[0]
    lo, hi = torch.from_numpy(root[0, :3].copy()).cuda(), torch.from_numpy(root[0, 3:].copy()).cuda()
    diag = float(torch.linalg.norm(hi - lo))
    geom = torch.from_numpy(m.scene_triangles(cfg)[0]).cuda()
    stream = torch.cuda.Stream()
    pts = surface_points(N, geom, diag, 4)
    half = 0.01 * diag
    boxes = torch.cat([pts - half, pts + half], 1).contiguous()  # (n, 6): mn, mx
    radius = torch.full((N,), half, dtype=torch.float32, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    f32 = dict(dtype=torch.float32, device="cuda")
    out = {"any": torch.empty(N, **i32), "count": torch.empty(N, **i32), "kind": torch.empty(N * K_MAX, **i32),
           "index": torch.empty(N * K_MAX, **i32), "tests": torch.empty(N, **i32)}
    nb = {"dist2": torch.empty(N * K_MAX, **f32), "point": torch.empty(N * K_MAX * 3, **f32),
          "bary": torch.empty(N * K_MAX * 2, **f32)}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with m.Renderer(cfg) as r:
        q, info = r.queue_info(), r.scene_info()
        emit("# Conference stand-in, %d triangles, box diagonal %.2f, half-side %.2f; renderer 2048 x 2048 Whitted: "
             "level-1 queue %d rays" % (info["triangles"], diag, half, q["rayCap"][0]))

        def timed(call):
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        def overlap_arm(k, fields):
            ptrs = {"d_" + f: out[f].data_ptr() for f in fields}
            return lambda: r.overlap_boxes_device(boxes.data_ptr(), boxes.data_ptr() + 12, N, k, mn_stride=6, mx_stride=6,
                                                  stream=stream.cuda_stream, **ptrs)

        def neighbour_arm():
            ptrs = {"d_" + f: x.data_ptr() for f, x in nb.items()}
            ptrs.update({"d_" + f: out[f].data_ptr() for f in ("count", "kind", "index", "tests")})
            r.neighbours_device(pts.data_ptr(), N, K_MAX, d_dist=radius.data_ptr(), stream=stream.cuda_stream, **ptrs)

        arms = [("overlap_boxes_device, any only", overlap_arm(1, ("any", "tests")), "any"),
                ("overlap_boxes_device, count only", overlap_arm(1, ("count", "tests")), "count"),
                ("overlap_boxes_device, K = %d, count" % K_MAX, overlap_arm(K_MAX, tuple(out)), "count"),
                ("neighbours_device, K = %d, count, radius" % K_MAX, neighbour_arm, "count")]
        notes = {}
        for name, call, field in arms:  # (also the first warm-up round)
            out["count"].fill_(-1)
            out["any"].fill_(-1)
            torch.cuda.synchronize()
            timed(call)
            notes[name] = "   mean tests per box %8.1f   mean %s %.2f, largest %d" % (
                float(out["tests"].float().mean()), field, float(out[field].float().mean()), int(out[field].max()))
        for _ in range(a.warmup):
            for _, call, _ in arms:
                timed(call)
        ms = {name: [] for name, _, _ in arms}
        for _ in range(a.reps):
            for name, call, _ in arms:
                ms[name].append(timed(call))
        for name, _, _ in arms:
            x = ms[name]
            emit("%-42s %8.3f ms [%8.3f .. %8.3f]   %7.1f M / s%s" % (name, statistics.median(x), min(x), max(x),
                                                                   N / statistics.median(x) * 1e-3, notes[name]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
