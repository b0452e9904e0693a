"""What a triangle overlap query costs: overlap_triangles_device on 2^20 query triangles on the Conference
stand-in, with overlap_boxes_device on the same triangles' hulls beside it.

The triangles have edges of about a chair leg's length (1.5 % of the box diagonal): the first corner is one of
the `surface` points of tools/nearest_bench.py (random surface points moved by up to 1 % of the diagonal per
axis), the other two lie at that distance from it in random directions.  Arms:
  overlap_triangles_device, any only          the walk stops at a triangle's first acceptance
  overlap_triangles_device, count only        every accepted candidate met, no list
  overlap_triangles_device, K = 16, count     every field
  overlap_boxes_device on the hulls           the same three forms: the broad phase on the same objects

One process and one renderer (2048 x 2048, Whitted: a level-1 queue of 2^22 rays, one chunk per call);
everything resident beforehand, events on the caller's stream around each call, the arms alternating;
median and range of --reps rounds after --warmup warm-up rounds.  Beside the times the mean of `tests` per
query (overlap-function evaluations) and the mean count.  Before any timing the entry lists of a subsample
are compared with a Naive renderer's.

  python tools/triangle_overlap_bench.py [--reps 20] [--warmup 3] [--out profiles/triangle_overlap_bench.txt]
"""
import argparse
import dataclasses
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import mobileraytracer_amd as m  # noqa: E402
from mobileraytracer_amd import _native  # noqa: E402
from nearest_bench import surface_points  # noqa: E402
from ray_query_bench import config  # noqa: E402

N = 1 << 20
K_MAX = 16
CHECKED = 2048  # the subsample compared with Naive


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
    emit("# python tools/triangle_overlap_bench.py " + " ".join(sys.argv[1:]))
    emit("# library %s (sources in the tree: %s)" % (_native.lib().mrt_build_stamp().decode(), _native.source_stamp()))
    emit("# overlap_triangles_device and overlap_boxes_device on the hulls, n = 2^20 triangles near the surfaces, events on")
    emit("# the caller's stream, one process, the arms alternating; median [least .. largest] of %d rounds after %d warm-up rounds"
         % (a.reps, a.warmup))
    cfg = config()
    root = m.triangle_bvh(cfg)[0]
    lo, hi = torch.from_numpy(root[0, :3].copy()).cuda(), torch.from_numpy(root[0, 3:].copy()).cuda()
    diag = float(torch.linalg.norm(hi - lo))
    geom = torch.from_numpy(m.scene_triangles(cfg)[0]).cuda()
    stream = torch.cuda.Stream()
    edge = 0.015 * diag
    g = torch.Generator(device="cuda").manual_seed(5)
    c0 = surface_points(N, geom, diag, 4)
    d = torch.randn((N, 2, 3), device="cuda", generator=g)
    d = d / torch.linalg.norm(d, dim=2, keepdim=True) * edge
    tris = torch.cat([c0, c0 + d[:, 0], c0 + d[:, 1]], 1).contiguous()  # (n, 9): a, b, c
    corners = tris.reshape(N, 3, 3)
    boxes = torch.cat([corners.min(1).values, corners.max(1).values], 1).contiguous()  # (n, 6): the hulls
    i32 = dict(dtype=torch.int32, device="cuda")
    out = {"any": torch.empty(N, **i32), "count": torch.empty(N, **i32), "kind": torch.empty(N * K_MAX, **i32),
           "index": torch.empty(N * K_MAX, **i32), "tests": torch.empty(N, **i32)}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with m.Renderer(cfg) as r:
        q, info = r.queue_info(), r.scene_info()
        emit("# Conference stand-in, %d triangles, box diagonal %.2f, edge length %.2f; renderer 2048 x 2048 Whitted: "
             "level-1 queue %d rays" % (info["triangles"], diag, edge, q["rayCap"][0]))
        sub = tris[:: N // CHECKED].contiguous()
        fields = ("any", "count", "kind", "index")
        fast = r.overlap_triangles(sub, K_MAX, fields=fields)
        with m.Renderer(dataclasses.replace(cfg, accelerator=1, width=64, height=64)) as naive:
            slow = naive.overlap_triangles(sub, K_MAX, fields=fields)
        torch.cuda.synchronize()
        for f in fields:
            if not torch.equal(fast[f], slow[f]):
                raise SystemExit("BVH and Naive differ in %s on the subsample" % f)
        emit("# checked before timing: any, count, kind and index of %d of the triangles equal a Naive renderer's "
             "(mean count %.2f)" % (len(sub), float(fast["count"].float().mean())))

        def timed(call):
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        def triangle_arm(k, wanted):
            ptrs = {"d_" + f: out[f].data_ptr() for f in wanted}
            base = tris.data_ptr()
            return lambda: r.overlap_triangles_device(base, base + 12, base + 24, N, k, a_stride=9, b_stride=9, c_stride=9,
                                                      stream=stream.cuda_stream, **ptrs)

        def box_arm(k, wanted):
            ptrs = {"d_" + f: out[f].data_ptr() for f in wanted}
            return lambda: r.overlap_boxes_device(boxes.data_ptr(), boxes.data_ptr() + 12, N, k, mn_stride=6, mx_stride=6,
                                                  stream=stream.cuda_stream, **ptrs)

        arms = []
        for who, arm in (("overlap_triangles_device", triangle_arm), ("overlap_boxes_device, hulls", box_arm)):
            arms += [(who + ", any only", arm(1, ("any", "tests")), "any"),
                     (who + ", count only", arm(1, ("count", "tests")), "count"),
                     (who + ", K = %d, count" % K_MAX, arm(K_MAX, tuple(out)), "count")]
        notes = {}
        for name, call, field in arms:  # (also the first warm-up round)
            out["count"].fill_(-1)
            out["any"].fill_(-1)
            torch.cuda.synchronize()
            timed(call)
            notes[name] = "   mean tests per query %8.1f   mean %s %.2f, largest %d" % (
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
            emit("%-44s %8.3f ms [%8.3f .. %8.3f]   %7.1f M / s%s" % (name, statistics.median(x), min(x), max(x),
                                                                     N / statistics.median(x) * 1e-3, notes[name]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
