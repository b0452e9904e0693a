"""What a full-visit multi-hit walk costs next to the exact closest-hit walk: cast_multi_hits_device at
K = 1, 4 and 16 against cast_rays_device on the rays of tools/ray_query_bench.py (Conference stand-in,
2^20 coherent camera rays and 2^20 incoherent ones), resident in device memory.

The arms alternate in one process, each timed with events on the caller's stream around the enqueued
work (the calls do not synchronise; the second event is waited for); medians and ranges of --rounds
rounds after --warmup warm-up rounds.  Before anything is timed, entry 0 of every multi-hit arm is
compared with cast_rays_device's closest hit (kind, index, the bits of t) and the arms' counts with each
other.  The mean count says how many accepted hits a ray has: the closest-hit walk stops caring after
the first, the multi-hit walk visits every box the ray passes and tests every triangle in them.

  python tools/multi_hit_bench.py [--rounds 20] [--warmup 3] [--out profiles/multi_hit_bench.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N = 1 << 20
KS = (1, 4, 16)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--out", default="")
    a = p.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit("# python tools/multi_hit_bench.py " + " ".join(sys.argv[1:]))

    import torch
    import mobileraytracer_amd as m
    from mobileraytracer_amd import _native
    import ray_query_bench as Q
    cfg = Q.config()
    boxes = m.triangle_bvh(cfg)[0]
    lo, hi = torch.from_numpy(boxes[0, :3].copy()).cuda(), torch.from_numpy(boxes[0, 3:].copy()).cuda()
    stream = torch.cuda.Stream()
    with m.Renderer(cfg) as r:
        q, info = r.queue_info(), r.scene_info()
        emit("# library %s; Conference stand-in, %d triangles; renderer %d x %d Whitted: level-1 queue %d rays"
             % (_native.lib().mrt_build_stamp().decode(), info["triangles"], Q.SIDE, Q.SIDE, q["rayCap"][0]))
        emit("# %d rays per call; events on the caller's stream around each call, arms alternating, %d rounds after %d"
             " warm-up rounds" % (N, a.rounds, a.warmup))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def timed(call):
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        for name, (o, d) in (("coherent", Q.coherent(N)), ("incoherent", Q.incoherent(N, lo, hi, 7))):
            ref = {"kind": torch.empty(N, dtype=torch.int32, device="cuda"),
                   "index": torch.empty(N, dtype=torch.int32, device="cuda"),
                   "t": torch.empty(N, dtype=torch.float32, device="cuda")}
            out = {k: {"count": torch.empty(N, dtype=torch.int32, device="cuda"),
                       "kind": torch.empty((N, k), dtype=torch.int32, device="cuda"),
                       "index": torch.empty((N, k), dtype=torch.int32, device="cuda"),
                       "t": torch.empty((N, k), dtype=torch.float32, device="cuda"),
                       "bary": torch.empty((N, k, 2), dtype=torch.float32, device="cuda")} for k in KS}
            torch.cuda.synchronize()

            def cast():
                r.cast_rays_device(o.data_ptr(), d.data_ptr(), N, d_kind=ref["kind"].data_ptr(),
                                   d_index=ref["index"].data_ptr(), d_t=ref["t"].data_ptr(), stream=stream.cuda_stream)

            def multi(k):
                def call():
                    r.cast_multi_hits_device(o.data_ptr(), d.data_ptr(), N, k, stream=stream.cuda_stream,
                                             **{"d_" + f: x.data_ptr() for f, x in out[k].items()})
                return call

            arms = [("cast_rays", cast)] + [("multi K=%d" % k, multi(k)) for k in KS]
            times = {arm: [] for arm, _ in arms}
            for rnd in range(1 + a.warmup + a.rounds):
                for arm, call in arms:
                    ms = timed(call)
                    if rnd > a.warmup:
                        times[arm].append(ms)
                if rnd == 0:  # the check: entry 0 is the closest-hit query, the counts agree
                    for k in KS:
                        for f in ("kind", "index", "t"):
                            if not torch.equal(out[k][f][:, 0].contiguous().view(torch.int32), ref[f].view(torch.int32)):
                                raise SystemExit("%s, K = %d: entry 0's %s differs from cast_rays_device" % (name, k, f))
                        if not torch.equal(out[k]["count"], out[KS[0]]["count"]):
                            raise SystemExit("%s, K = %d: count differs from K = %d's" % (name, k, KS[0]))
            count = out[KS[-1]]["count"].float()
            emit("# %s: %.1f %% of the rays hit; entry 0 equals cast_rays_device at K = 1, 4, 16; count: mean %.2f, max %d,"
                 " %.1f %% of the rays above 16" % (name, 100.0 * float((ref["kind"] > 0).float().mean()), float(count.mean()),
                                                     int(count.max()), 100.0 * float((count > 16).float().mean())))
            base = statistics.median(times["cast_rays"])
            for arm, _ in arms:
                ms = times[arm]
                emit("%-11s %-11s median %8.3f  min %8.3f  max %8.3f ms  %7.1f M rays/s  %6.2f x cast_rays"
                     % (name, arm, statistics.median(ms), min(ms), max(ms), N / statistics.median(ms) * 1e-3,
                        statistics.median(ms) / base))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
