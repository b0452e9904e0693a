"""What a batch of views buys: render_views_device against the sequential loop of set_camera +
render_frame_device over the same K = 8 cameras (an arc around the Conference stand-in's camera),
PathTracer, depth 5, 4 spp, at a C4-shard-sized frame (480 x 272) and at the full 1920 x 1080.

One process; the two arms alternate, each timed window closed by a device synchronise; the bitmaps of
the two arms are compared before anything is timed.  Each arm has a renderer of its own: the queue
plan is sized for the slot range a pass runs over, so one renderer alternating between frames and
batches would re-allocate its queues at every switch.

  python tools/views_ab.py [--batches 20] [--out profiles/views_batch_ab.txt]
  python tools/views_ab.py --sequential-only      # a build without mrt_render_views (the parent's)
"""
import argparse
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import mobileraytracer_amd as m  # noqa: E402
from mobileraytracer_amd import scenes  # noqa: E402

K = 8
SIZES = ((480, 272), (1920, 1080))


def orbit(width, height):
    """K cameras on an arc (5 degrees apart) around conference.cam's look-at point, at its height and
    distance: (kind, position, look_at, up, hFov, vFov) as loadCameraStream makes them."""
    px, py, pz = 460.0, 500.0, -1000.0  # conference.cam's position, X negated
    look = (0.0, 400.0, 0.0)
    radius, base = math.hypot(px, pz), math.atan2(pz, px)
    cams = []
    for k in range(K):
        a = base + math.radians(5.0 * (k - (K - 1) / 2))
        cams.append((0, (radius * math.cos(a), py, radius * math.sin(a)), look, (0.0, 1.0, 0.0),
                     45.0 * width / height, 45.0))
    return cams


def renderer(width, height):
    o, l, c = scenes.conference()
    return m.Renderer(m.Config(width=width, height=height, shader=2, sceneIndex=-1, samplesPixel=4, maxDepth=5,
                               objFilePath=o, mtlFilePath=l, camFilePath=c))


def summary(name, ms):
    return "%-10s median %8.3f  min %8.3f  max %8.3f ms per %d views  (%d rounds)" % (
        name, statistics.median(ms), min(ms), max(ms), K, len(ms))


def measure(width, height, batches, warmup, sequential_only, emit):
    cams = orbit(width, height)
    n = width * height
    stream = torch.cuda.current_stream().cuda_stream
    seq = renderer(width, height)
    bat = None if sequential_only else renderer(width, height)
    d_seq = torch.zeros((K, n), dtype=torch.int32, device="cuda")
    d_bat = torch.zeros((K, n), dtype=torch.int32, device="cuda")

    def run_seq():
        for v, cam in enumerate(cams):
            seq.set_camera(*cam)
            seq.render_frame_device(d_seq[v].data_ptr(), 0, stream)
        torch.cuda.synchronize()

    def run_bat():
        bat.render_views_device(cams, d_bat.data_ptr(), 0, stream)
        torch.cuda.synchronize()

    try:
        run_seq()
        rays = seq.get_total_casted_rays()
        emit("%dx%d  PathTracer depth 5, 4 spp, K = %d views, %d rays per %d views" % (width, height, K, rays, K))
        if bat is not None:
            run_bat()
            same = bool(torch.equal(d_seq, d_bat)) and bat.get_total_casted_rays() == rays
            emit("  bitmaps and ray counts of the two arms identical: %s" % same)
            if not same:
                raise SystemExit("the batch differs from the sequential loop")
            q = bat.queue_info()
            emit("  batch plan: chunkSlots %d, passes %d" % (q["chunkSlots"], q["passes"]))
        for _ in range(warmup):
            run_seq()
            if bat is not None:
                run_bat()
        t_seq, t_bat = [], []
        for _ in range(batches):
            t0 = time.perf_counter()
            run_seq()
            t_seq.append((time.perf_counter() - t0) * 1e3)
            if bat is not None:
                t0 = time.perf_counter()
                run_bat()
                t_bat.append((time.perf_counter() - t0) * 1e3)
        emit("  " + summary("sequential", t_seq))
        if bat is not None:
            emit("  " + summary("batch", t_bat))
            emit("  batch / sequential (medians): %.3f   (minima): %.3f" % (
                statistics.median(t_bat) / statistics.median(t_seq), min(t_bat) / min(t_seq)))
    finally:
        seq.close()
        if bat is not None:
            bat.close()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batches", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--sequential-only", action="store_true")
    p.add_argument("--out", default="")
    a = p.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit("# tools/views_ab.py: render_views_device vs the loop of set_camera + render_frame_device, one process,")
    emit("# alternating, %d rounds after %d warm-up rounds, a device synchronise closing each window" % (a.batches, a.warmup))
    for w, h in SIZES:
        measure(w, h, a.batches, a.warmup, a.sequential_only, emit)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


main()
