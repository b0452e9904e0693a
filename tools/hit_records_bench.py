"""What a surface record costs on top of a hit: cast_hits_device against cast_rays_device on the same
rays - the C4 frame's own camera rays at 1 spp (Conference stand-in, 1920 x 1080; the export is not
timed), resident in device memory.

Four arms, alternating in one process, each timed with events on the caller's stream around the
enqueued work (the calls do not synchronise; the second event is waited for):
  cast_rays        cast_rays_device: kind, index, t                     (k_query_store)
  hits kit         cast_hits_device with only kind / index / t set: the same launches as cast_rays
  hits geometry    ... with kind, index, t, bary, point                 (k_query_store_hits<false>)
  hits full        ... with all thirteen fields                         (k_query_store_hits<true>)
Before anything is timed the arms' common fields are compared.

The store kernels' traffic per ray is computed here from the record sizes: `streamed` is what every
ray reads from the level-1 queue and writes to the outputs, `gathered` what a triangle hit reads from
the scene's tables on top (cache-resident for a scene's working set).  Their time is not visible to
events around a whole call, so the achieved bandwidth comes from a kernel trace of a run of this tool:

  python tools/hit_records_bench.py [--rounds 20] [--warmup 3] [--out profiles/hit_records_bench.txt]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/hit_records_bench.py --out LOG
  python tools/hit_records_bench.py --stats DIR/.../run_kernel_stats.csv --log LOG      (needs no GPU)

--only cast times cast_rays_device alone; with MOBILERT_LIB naming a build of the parent commit that is
the parent's own figure, and two such runs around a run of this tree give the spread the `hits kit`
arm is judged against (it launches the parent's kernels, so a difference beyond that spread is a defect).
"""
import argparse
import csv
import os
import re
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIDTH, HEIGHT = 1920, 1080
FIELD_BYTES = {"kind": 4, "index": 4, "t": 4, "bary": 8, "point": 12, "normal": 12, "texCoord": 8, "material": 4,
               "kd": 12, "ks": 12, "kt": 12, "le": 12, "ior": 4}
KIT = ("kind", "index", "t")
GEOMETRY = KIT + ("bary", "point")
FULL = tuple(FIELD_BYTES)
# per ray: the queue records read (hit; the geometry and full kernels also rO and rD) and the order table's entry
STREAMED_IN = {"store": 16 + 4, "geometry": 48 + 4, "full": 48 + 4}
# per triangle hit of an untextured scene: triHead 16 B, the material's four records 64 B (a smooth
# triangle: nB, nC 32 B more; a textured scene: triTex 32 B, the material word 16 B and the texel)
GATHERED = {"store": 0, "geometry": 0, "full": 16 + 64}
KERNELS = {"store": r"k_query_store\(", "geometry": r"k_query_store_hits<false>", "full": r"k_query_store_hits<true>"}


def streamed(kernel):
    out = {"store": KIT, "geometry": GEOMETRY, "full": FULL}[kernel]
    return STREAMED_IN[kernel] + sum(FIELD_BYTES[f] for f in out)


def summary(name, ms):
    return "%-14s median %8.3f  min %8.3f  max %8.3f ms  (%d rounds)" % (name, statistics.median(ms), min(ms), max(ms), len(ms))


def from_stats(path, log, emit):
    """Achieved bandwidth of the store kernels from rocprofv3's kernel statistics of a run whose log
    (--out) says how many rays went through each."""
    rays = {}
    with open(log) as f:
        for line in f:
            found = re.match(r"# kernel rays: (.*)", line)
            if found:
                rays = {k: int(v) for k, v in (kv.split("=") for kv in found.group(1).split())}
    if not rays:
        raise SystemExit("%s has no '# kernel rays:' line" % log)
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    for kernel, pattern in KERNELS.items():
        ns = sum(int(r["TotalDurationNs"]) for r in rows if re.search(pattern, r["Name"]))
        calls = sum(int(r["Calls"]) for r in rows if re.search(pattern, r["Name"]))
        if ns == 0 or rays.get(kernel, 0) == 0:
            emit("%-9s not in the trace" % kernel)
            continue
        s, g = streamed(kernel), GATHERED[kernel]
        emit("%-9s %5d launches, %7.1f us each, %6.3f ns/ray: %3d B/ray streamed = %7.1f GB/s (with %d B gathered per hit: %7.1f GB/s)"
             % (kernel, calls, ns / calls * 1e-3, ns / rays[kernel], s, s * rays[kernel] / ns, g, (s + g) * rays[kernel] / ns))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--only", choices=("cast",), default=None)
    p.add_argument("--out", default="")
    p.add_argument("--stats", default="")
    p.add_argument("--log", default="")
    a = p.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit("# python tools/hit_records_bench.py " + " ".join(sys.argv[1:]))
    if a.stats:
        from_stats(a.stats, a.log, emit)
        return 0

    import torch
    import mobileraytracer_amd as m
    from mobileraytracer_amd import _native, scenes
    o, l, c = scenes.conference()
    cfg = m.Config(width=WIDTH, height=HEIGHT, shader=2, sceneIndex=-1, samplesPixel=4, maxDepth=5, objFilePath=o,
                   mtlFilePath=l, camFilePath=c)
    stream = torch.cuda.Stream()
    with m.Renderer(cfg) as r:
        orig, dirs, _, _ = r.camera_rays(spp=1)
        n = orig.shape[0]
        q, info = r.queue_info(), r.scene_info()
        chunks = -(-n // q["rayCap"][0])
        emit("# library %s; Conference stand-in, %d triangles, C4 frame %d x %d: %d camera rays at 1 spp, level-1 queue %d"
             " rays: %d chunk(s) per call" % (_native.lib().mrt_build_stamp().decode(), info["triangles"], WIDTH, HEIGHT, n,
                                               q["rayCap"][0], chunks))
        emit("# events on the caller's stream around each call, arms alternating, %d rounds after %d warm-up rounds"
             % (a.rounds, a.warmup))
        out = {}
        for f, width in FIELD_BYTES.items():
            dtype = torch.int32 if f in ("kind", "index", "material") else torch.float32
            out[f] = torch.empty(n * width // 4, dtype=dtype, device="cuda")
        ref = {f: torch.empty_like(out[f]) for f in KIT}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()

        def timed(call):
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        def cast():
            r.cast_rays_device(orig.data_ptr(), dirs.data_ptr(), n, d_kind=ref["kind"].data_ptr(),
                               d_index=ref["index"].data_ptr(), d_t=ref["t"].data_ptr(), stream=stream.cuda_stream)

        def records(fields):
            def call():
                r.cast_hits_device(orig.data_ptr(), dirs.data_ptr(), n, stream=stream.cuda_stream,
                                   **{"d_" + f: out[f].data_ptr() for f in fields})
            return call

        arms = [("cast_rays", cast, "store")]
        if a.only is None:
            arms += [("hits kit", records(KIT), "store"), ("hits geometry", records(GEOMETRY), "geometry"),
                     ("hits full", records(FULL), "full")]
        through = {"store": 0, "geometry": 0, "full": 0}
        times = {name: [] for name, _, _ in arms}
        for k in range(1 + a.warmup + a.rounds):
            for name, call, kernel in arms:
                ms = timed(call)
                through[kernel] += n
                if k == 0 and name != "cast_rays":  # the check: the arms agree on what they share
                    for f in KIT:
                        if not torch.equal(out[f].view(torch.int32), ref[f].view(torch.int32)):
                            raise SystemExit("%s: %s differs from cast_rays_device" % (name, f))
                    out["kind"].fill_(-1)
                    torch.cuda.synchronize()
                if k > a.warmup:
                    times[name].append(ms)
        hit = float((ref["kind"] > 0).float().mean())
    emit("# %.1f %% of the rays hit; the arms' kind / index / t agree" % (100.0 * hit))
    base = statistics.median(times["cast_rays"])
    for name, _, kernel in arms:
        extra = "" if name == "cast_rays" else "  %+8.3f ms vs cast_rays (%.3f x)" % (
            statistics.median(times[name]) - base, statistics.median(times[name]) / base)
        emit(summary(name, times[name]) + "  %7.1f M rays/s" % (n / statistics.median(times[name]) * 1e-3) + extra)
    for kernel in ("store", "geometry", "full"):
        emit("# %-9s kernel: %3d B/ray streamed (queue records in, outputs out), %d B gathered per triangle hit"
             % (kernel, streamed(kernel), GATHERED[kernel]))
    emit("# kernel rays: " + " ".join("%s=%d" % kv for kv in through.items()))
    emit("# the store kernels' own time and GB/s: --stats on a rocprofv3 kernel trace of this run")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


sys.exit(main())
