"""What the resident ray query buys: cast_rays_device (rays and results in device memory, ordered on
the caller's stream) against trace_rays from host arrays (the only way to trace one's own rays
before it), on the Conference stand-in.

Closest hit and any hit, 2^20 and 2^24 rays, two ray sets:
  coherent    the scene camera's own pinhole rays (position, look-at, up and fields of view read from
              the scene's .cam file), one per pixel of a square grid;
  incoherent  origins uniform in the scene's bounding box, directions uniform on the sphere.
Any hit: tmax uniform in (0, the box diagonal).

One process and one renderer (2048 x 2048, Whitted: a level-1 queue of 2^22 rays, so the large
batches run in four chunks on either path); the two paths alternate.  The resident path is timed
with events on the caller's stream around the call, everything resident beforehand; the host path
with the host clock around the call, which ends synchronised with its results on the host.  Their
results are compared before anything is timed.

  python tools/ray_query_bench.py [--reps 20] [--out profiles/ray_query_bench.txt]
"""
import argparse
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mobileraytracer_amd as m  # noqa: E402
from mobileraytracer_amd import scenes  # noqa: E402

SIZES = (1 << 20, 1 << 24)
SIDE = 2048


def config():
    o, l, c = scenes.conference()
    return m.Config(width=SIDE, height=SIDE, shader=1, sceneIndex=-1, objFilePath=o, mtlFilePath=l, camFilePath=c)


def scene_camera():
    """position, look-at, up and the two fields of view in degrees of the scene's .cam file, read as
    the renderer's loader reads it (the position's X negated)."""
    cam = {}
    with open(scenes.conference()[2]) as f:
        for line in f:
            line = line.split("#")[0].split()
            if line and line[0] in ("p", "l", "u", "f"):
                cam[line[0]] = [float(x) for x in line[1:]]
    cam["p"][0] = -cam["p"][0]
    return cam["p"], cam["l"], cam["u"], cam["f"]


def coherent(n):
    """Pinhole rays of the scene's own camera (scene_camera; a square image, so the horizontal field
    of view is the file's), one through the centre of every pixel of a sqrt(n) x sqrt(n) grid,
    row-major.  (The renderer's camera rays add the pixel jitter; these are as coherent.)"""
    side = int(math.isqrt(n))
    assert side * side == n
    p, l, u, f = scene_camera()
    pos = torch.tensor(p, device="cuda")
    fwd = torch.nn.functional.normalize(torch.tensor(l, device="cuda") - pos, dim=0)
    right = torch.nn.functional.normalize(torch.linalg.cross(torch.tensor(u, device="cuda"), fwd), dim=0)
    up = torch.linalg.cross(fwd, right)
    s = (torch.arange(side, device="cuda", dtype=torch.float32) + 0.5) / side * 2.0 - 1.0
    v, u = torch.meshgrid(-s * math.tan(math.radians(f[1] / 2)), s * math.tan(math.radians(f[0] / 2)), indexing="ij")
    d = fwd + u.reshape(-1, 1) * right + v.reshape(-1, 1) * up
    return pos.expand(n, 3).contiguous(), torch.nn.functional.normalize(d, dim=1).contiguous()


def incoherent(n, lo, hi, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    o = lo + torch.rand((n, 3), device="cuda", generator=g) * (hi - lo)
    d = torch.nn.functional.normalize(torch.randn((n, 3), device="cuda", generator=g), dim=1)
    return o.contiguous(), d.contiguous()


def row(r, name, n, any_hit, o, d, dist, reps, warmup, stream, emit):
    ho, hd, hdist = o.cpu().numpy(), d.cpu().numpy(), dist.cpu().numpy()
    k = torch.empty(n, dtype=torch.int32, device="cuda")
    i = torch.empty(n, dtype=torch.int32, device="cuda")
    t = torch.empty(n, dtype=torch.float32, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()

    def resident():
        e0.record(stream)
        r.cast_rays_device(o.data_ptr(), d.data_ptr(), n, d_dist=dist.data_ptr() if any_hit else 0, any_hit=any_hit,
                           d_kind=k.data_ptr(), d_index=0 if any_hit else i.data_ptr(), d_t=0 if any_hit else t.data_ptr(),
                           stream=stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    def host():
        t0 = time.perf_counter()
        res = r.trace_rays(ho, hd, dist=hdist if any_hit else None, any_hit=any_hit)
        return time.perf_counter() - t0, res

    resident()
    _, ref = host()
    same = np.array_equal(k.cpu().numpy(), ref[0])
    if not any_hit:
        same = same and np.array_equal(i.cpu().numpy(), ref[1]) and np.array_equal(
            t.cpu().numpy().view(np.int32), ref[2].view(np.int32))
    if not same:
        raise SystemExit("%s: the resident path differs from the host path" % name)
    share = float((ref[0] > 0).mean())
    for _ in range(warmup):
        resident()
        host()
    t_res, t_host = [], []
    for _ in range(reps):
        t_res.append(resident())
        t_host.append(host()[0])
    a, b = statistics.median(t_res), statistics.median(t_host)
    emit("%-11s %-10s n = 2^%d  %s %5.1f %%   resident %9.1f M rays/s (%8.3f ms)   host arrays %8.1f M rays/s (%9.3f ms)"
         "   resident / host: %6.1fx" % ("any hit" if any_hit else "closest hit", name, n.bit_length() - 1,
                                         "occluded" if any_hit else "hit     ", 100.0 * share, n / a * 1e-6, a * 1e3,
                                         n / b * 1e-6, b * 1e3, b / a))
    return b / a


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default="")
    a = p.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit("# python tools/ray_query_bench.py " + " ".join(sys.argv[1:]))
    emit("# cast_rays_device (resident, events on the caller's stream) vs trace_rays (host arrays, host clock), one")
    emit("# process, alternating, medians of %d repetitions after %d warm-up rounds" % (a.reps, a.warmup))
    cfg = config()
    boxes = m.triangle_bvh(cfg)[0]
    lo, hi = torch.from_numpy(boxes[0, :3].copy()).cuda(), torch.from_numpy(boxes[0, 3:].copy()).cuda()
    diag = float(torch.linalg.norm(hi - lo))
    stream = torch.cuda.Stream()
    ratios = []
    with m.Renderer(cfg) as r:
        q, info = r.queue_info(), r.scene_info()
        emit("# coherent rays: the camera of %s: position %s, look-at %s, up %s, fov %s"
             % ((os.path.basename(scenes.conference()[2]),) + scene_camera()))
        emit("# Conference stand-in, %d triangles; renderer %d x %d Whitted: level-1 queue %d rays, %d shadow rays"
             % (info["triangles"], SIDE, SIDE, q["rayCap"][0], q["shadowCap"][0]))
        for any_hit in (False, True):
            for n in SIZES:
                for name, (o, d) in (("coherent", coherent(n)), ("incoherent", incoherent(n, lo, hi, 7))):
                    g = torch.Generator(device="cuda").manual_seed(9)
                    dist = torch.rand(n, device="cuda", generator=g) * diag
                    ratios.append(row(r, name, n, any_hit, o, d, dist, a.reps, a.warmup, stream, emit))
    emit("# the resident path is not slower on any row: %s (least ratio %.1fx)" % (min(ratios) >= 1.0, min(ratios)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if min(ratios) >= 1.0 else 1


if __name__ == "__main__":  # (tools/multi_hit_bench.py imports the ray generators)
    sys.exit(main())
