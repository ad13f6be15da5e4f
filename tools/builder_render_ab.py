"""S2 at 1080p: ms per 16 spp call (8 pipelined calls + sync) and build ms, the three builders (host SAH, GPU LBVH, GPU PLOC)
alternating in one process, five passes each after a warm-up pass."""
import sys, time, statistics
sys.path.insert(0, '.')
from computeraytracer_amd import Renderer, scenes_synth
r = Renderer(0)
r.upload(scenes_synth.atrium250k(1920, 1080))
def run():
    r.reset(); r.sync()
    t0 = time.perf_counter()
    for _ in range(8): r.frame(16)
    r.sync()
    return (time.perf_counter() - t0) * 1e3 / 8
ts = {m: [] for m in ('bvh2', 'lbvh', 'ploc')}
builds = {m: [] for m in ts}
for p in range(6):
    for m in ts:
        t0 = time.perf_counter(); r.build_accel(m); b = (time.perf_counter() - t0) * 1e3
        v = run()
        if p: ts[m].append(v); builds[m].append(b)       # pass 0 warms up
for m in ts:
    print('%-5s render ms per 16 spp: median %.2f min %.2f max %.2f | build ms: median %.2f min %.2f' %
          (m, statistics.median(ts[m]), min(ts[m]), max(ts[m]), statistics.median(builds[m]), min(builds[m])), flush=True)
