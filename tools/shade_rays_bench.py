"""What radiance per ray costs against radiance per pixel: shade_rays_device on the renderer's own
exported camera rays (the export is not timed) against render_frame_device of the same frame, on the
Conference stand-in, PathTracer, depth 5, 4 spp, at the full 1920 x 1080 and at a C4-shard-sized
480 x 272.

The two do the same work below level 1.  The batch form reads 28 B (origin, direction, key) and writes
12 B per ray more than the frame, whose level 1 is generated in the walk and folded into 8-bit pixels,
and it runs level 1 unfused from stored records (load, packet walk, k_shade, k_resolve_store).

One process; the two arms alternate, each call host-synchronous (it returns with its output written),
timed with the host clock.  Each arm has a renderer of its own: the queue plan is sized for the slot
range a pass runs over, so one renderer alternating between frames and batches would re-allocate its
queues at every switch.  Before anything is timed the batch's radiance, folded per pixel by the
library's accumulation kernel (kat_accumulate: incrementalAvg in sample order), must equal the
frame's bitmap.

  python tools/shade_rays_bench.py [--rounds 20] [--out profiles/shade_rays_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mobileraytracer_amd as m  # noqa: E402
from mobileraytracer_amd import scenes  # noqa: E402

SIZES = ((1920, 1080), (480, 272))
SPP = 4


def renderer(width, height):
    o, l, c = scenes.conference()
    return m.Renderer(m.Config(width=width, height=height, shader=2, sceneIndex=-1, samplesPixel=SPP, maxDepth=5,
                               objFilePath=o, mtlFilePath=l, camFilePath=c))


def summary(name, ms):
    return "%-18s median %8.3f  min %8.3f  max %8.3f ms  (%d rounds)" % (
        name, statistics.median(ms), min(ms), max(ms), len(ms))


def size(width, height, rounds, warmup, emit):
    with renderer(width, height) as rf, renderer(width, height) as rs:
        bitmap = torch.zeros(width * height, dtype=torch.int32, device="cuda")
        orig, dirs, keys, _ = rs.camera_rays()
        n = orig.shape[0]  # pixelSlots x spp (the frame's tiles may leave a remainder of the pixels out)
        rgb = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def frame():
            t0 = time.perf_counter()
            rf.render_frame_device(bitmap.data_ptr())
            return (time.perf_counter() - t0) * 1e3

        def shade():
            t0 = time.perf_counter()
            rays = rs.shade_rays_device(orig.data_ptr(), dirs.data_ptr(), n, d_key=keys.data_ptr(), d_rgb=rgb.data_ptr())
            return (time.perf_counter() - t0) * 1e3, rays

        frame()
        _, rays = shade()
        torch.cuda.synchronize()
        want = bitmap.cpu().numpy()
        folded = np.zeros(width * height, np.int32)
        m.kat_accumulate(rgb.cpu().numpy(), SPP, 0, folded, width, height)
        st = rf.frame_stats()
        if not np.array_equal(folded, want) or rays != (st["rays"], st["shadowRays"]):
            raise SystemExit("%d x %d: the folded batch differs from the frame (%d pixels; rays %s vs %s)" % (
                width, height, int((folded != want).sum()), rays, (st["rays"], st["shadowRays"])))
        for _ in range(warmup):
            frame()
            shade()
        t_frame, t_shade = [], []
        for _ in range(rounds):
            t_frame.append(frame())
            t_shade.append(shade()[0])
    a, b = statistics.median(t_frame), statistics.median(t_shade)
    emit("%d x %d, %d spp: %d level-1 rays, %d rays and %d shadow rays per call; folded batch == frame: True"
         % (width, height, SPP, n, rays[0], rays[1]))
    emit("  " + summary("render_frame_device", t_frame))
    emit("  " + summary("shade_rays_device", t_shade))
    emit("  shade / frame: %.3f  (%.1f vs %.1f M level-1 rays/s)" % (b / a, n / b * 1e-3, n / a * 1e-3))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=20)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default="")
    a = p.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit("# python tools/shade_rays_bench.py " + " ".join(sys.argv[1:]))
    emit("# shade_rays_device on the exported camera rays vs render_frame_device of the same frame: Conference")
    emit("# stand-in, PathTracer, depth 5, %d spp; one process, a renderer per arm, alternating, host clock around" % SPP)
    emit("# host-synchronous calls, %d rounds after %d warm-up rounds; the ratio is recorded, not a target" % (a.rounds, a.warmup))
    for width, height in SIZES:
        size(width, height, a.rounds, a.warmup, emit)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


sys.exit(main())
