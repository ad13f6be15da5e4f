"""Scene edits (include/crt.h "Scene edits") on S2 (atrium250k) at 1920 x 1080 and on the 10 M-triangle soup: host clock
around synchronous calls, warm, median of --reps.

  build_lbvh_ms        crt_build_accel(CRT_ACCEL_LBVH)
  build_ploc_ms        crt_build_accel(CRT_ACCEL_PLOC)
  refit_ms             crt_refit_accel after a crt_update_primitives (the update itself not timed); option
                       "refit_rebuild_pct" = 0
  refit_policy_ms      the same with "refit_rebuild_pct" = 100000: the policy computes the tree's cost after every refit
                       and never fires; policy_added_ms = the difference
  quality_ms           crt_accel_quality
  update_ms            crt_update_primitives of the moved tenth (records, hit_pad reduction, state reset)
  transform_ms         crt_transform_primitives of the same tenth by the same rigid move, one op (the records never leave
                       the device; forward and inverse alternate so that the geometry stays where it is)
  transform_1000_ms    the same tenth as 1000 ops of one call
  refit_after_transform_ms   crt_refit_accel after such a call
  set_camera_ms        crt_set_camera with a pad that does not grow (no refit): sync + camera + state reset
  set_camera_refit_ms  crt_set_camera with an eye farther out each call (the pad grows: inline refit)
  step_ms_refit / step_ms_fresh / step_ms_fresh_ploc   ms per --spp step after a rigid move of a contiguous tenth of the
                       primitives, refitted tree against a fresh LBVH / PLOC build of the same buffers (the tree-quality cost)
  edit_total_ms        what one edited frame costs by each route: refit + step, LBVH rebuild + step, PLOC rebuild + step
  q_built / q_refit / q_fresh   Q = boxes + prims of the walked tree (crt_accel_quality): as built, after the rigid move of
                       the tenth and the refit, and of the fresh LBVH of the moved buffers; q_ratio = q_refit / q_built is
                       what "refit_rebuild_pct" compares, q_ratio_fresh = q_refit / q_fresh stands beside
                       step_ratio = step_ms_refit / step_ms_fresh

--parent DIR: a checkout of the parent commit with its library built.  Its crt_update_primitives of the same tenth is
and its crt_refit_accel after it are measured in child processes (this tool with --update-only --tree DIR) before and
after this build's run, in one session: parent_update_ms and parent_refit_ms hold both medians, their difference is the
run-to-run spread the comparison allows for.

--topology: crt_remove_primitives / crt_append_primitives instead (--out profiles/topology_edit_bench.json), the library
calls alone (the Renderer methods also restate the edit on the host copy of the scene, which is not the library's cost):
  remove_one_ms / remove_1000_ms     crt_remove_primitives of the last tenth as one range / as 1000 touching ranges
  append_ms                          crt_append_primitives of that tenth, back where it was (the record array still has the room)
  remove_mid_ms                      crt_remove_primitives of a tenth from the middle of a freshly uploaded scene (from n / 3 on:
                                     the host mirror moves everything behind it down and renumbers it; the tail range above
                                     moves nothing on the host)
  append_grow_ms                     the same into an array without room: a fresh upload, then the tenth appended (once per rep)
  rebuild_after_remove_ms / rebuild_after_append_ms   the rebuilding crt_refit_accel after each (LBVH)
  edit_rebuild_ms                    remove + rebuild and append + rebuild, the two sums
  upload_build_ms                    crt_upload_scene + crt_build_accel(LBVH) of the resulting buffers, this build: [without the
                                     tenth, with it]; parent_upload_build_ms (--parent): the parent commit's, before and after
  ratio                              edit_rebuild_ms / the parent's upload_build_ms (the faster of before / after), per edit

Per-kernel times come from a separate run under rocprofv3 --kernel-trace --stats.  Prints one JSON line; --out also
writes it.

The kernel times of the tree cost (profiles/quality_kernel_stats.csv) are made in two steps:
  rocprofv3 --kernel-trace --stats -d DIR -o quality -- python tools/refit_bench.py --policy-loop
      per scene: an LBVH build, "refit_rebuild_pct" = 100000, ten times crt_update_primitives of the tenth (the records
      it already holds) + crt_refit_accel, then one crt_accel_quality
  python tools/refit_bench.py --kernel-stats DIR/quality_results.db --out profiles/quality_kernel_stats.csv
      from the trace's `kernels` view: the dispatches of k_quality_nodes, k_quality_sum and k_refit_quant4 grouped by
      (kernel name as the trace spells it, grid threads): calls, mean / min / max of end - start in microseconds.  The
      grid tells the scenes and trees apart (a thread per node, blocks of 256); k_quality_sum, always one block, is
      listed under the grid of the k_quality_nodes launch before it, whose pairs it adds."""
import argparse
import json
import os
import statistics
import sys
import time

TREE = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(TREE))

import numpy as np  # noqa: E402

from computeraytracer_amd import Renderer  # noqa: E402
from computeraytracer_amd.scene import transform_records  # noqa: E402
from computeraytracer_amd.scenes_synth import atrium250k, soup  # noqa: E402


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(ts), 4)


def run_scene(name, ps, reps, spp, steps, update_only=False):
    n = len(ps.primitives)
    first, cnt = n // 3, n // 10
    th = 0.05
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    moved = ps.primitives.copy()
    moved[first:first + cnt] = transform_records(moved[first:first + cnt], R, [6.0, 2.0, -4.0])
    rec_a, rec_b = ps.primitives[first:first + cnt], moved[first:first + cnt]
    res = {"scene": name, "primitives": n, "moved": cnt, "width": ps.width, "height": ps.height, "reps": reps}
    r = Renderer(0)
    try:
        r.upload(ps)
        res["build_lbvh_ms"] = timed(lambda: r.build_accel("lbvh"), reps)
        if not update_only:
            res["build_ploc_ms"] = timed(lambda: r.build_accel("ploc"), reps)
            r.build_accel("lbvh")
        flip = [0]

        def update():
            flip[0] ^= 1
            r.update_primitives(first, rec_b if flip[0] else rec_a)

        res["update_ms"] = timed(update, reps)

        def refit_after_update():
            ts = []
            for _ in range(reps + 3):
                update()
                t = time.perf_counter()
                rebuilt = r.refit_accel()
                ts.append((time.perf_counter() - t) * 1e3)
                assert not rebuilt
            return round(statistics.median(ts[3:]), 4)

        res["refit_ms"] = refit_after_update()
        if update_only:
            return res
        r.set_option("refit_rebuild_pct", 100000)                        # the cost after every refit; never past 1000 x
        res["refit_policy_ms"] = refit_after_update()
        r.set_option("refit_rebuild_pct", 0)
        res["policy_added_ms"] = round(res["refit_policy_ms"] - res["refit_ms"], 4)
        res["quality_ms"] = timed(r.accel_quality, reps)
        if flip[0]:
            update()                                                     # the uploaded records again, for what follows
        r.build_accel("lbvh")
        from computeraytracer_amd.scene import transform_ops            # (a parent tree has none: imported past --update-only)
        t3 = np.float64([6.0, 2.0, -4.0])
        fwd = np.concatenate([R, t3[:, None]], 1).astype(np.float32).reshape(12)
        inv = np.concatenate([R.T, -(R.T @ t3)[:, None]], 1).astype(np.float32).reshape(12)
        bounds = np.linspace(first, first + cnt, 1001).astype(np.int64)
        # packed once, outside the timed region (transform_ops passes such an array through)
        many = [transform_ops([(int(a), int(b - a), m) for a, b in zip(bounds[:-1], bounds[1:])]) for m in (inv, fwd)]
        one = [transform_ops([(first, cnt, m)]) for m in (inv, fwd)]

        def transform(ops):
            def call():
                flip[0] ^= 1
                r.transform_primitives(ops[flip[0]])
            return call

        flip[0] = 0
        res["transform_ms"] = timed(transform(one), reps, warm=4)        # (an even number of calls: back where it began)
        res["transform_1000_ms"] = timed(transform(many), reps, warm=4)
        ts = []
        for _ in range(reps + 4):
            transform(one)()
            t = time.perf_counter()
            rebuilt = r.refit_accel()
            ts.append((time.perf_counter() - t) * 1e3)
            assert not rebuilt
        res["refit_after_transform_ms"] = round(statistics.median(ts[4:]), 4)
        r.update_primitives(first, rec_a)                                # the uploaded records again, for what follows
        assert not r.refit_accel()                                       # (a stale tree is not refitted inside set_camera)
        flip[0] = 0
        res["refit_speedup"] = round(res["build_lbvh_ms"] / res["refit_ms"], 2)
        cam0 = ps.camera.copy()
        look = cam0[4:7].astype(np.float64)
        v = cam0[0:3].astype(np.float64) - look
        near = [cam0.copy(), cam0.copy()]
        near[1][0:3] = (look + 0.9 * v).astype(np.float32)
        k = [0]

        def cam_near():
            k[0] ^= 1
            r.set_camera(near[k[0]])

        r.set_camera(cam0)
        res["set_camera_ms"] = timed(cam_near, reps)
        grow = [1.0]
        far_scale = 1e6 / max(np.linalg.norm(v), 1.0)

        def cam_far():
            grow[0] *= 1.01
            c = cam0.copy()
            c[0:3] = (look + far_scale * grow[0] * v).astype(np.float32)   # |eye| beyond the scene and growing: refit
            r.set_camera(c)

        res["set_camera_refit_ms"] = timed(cam_far, reps)
        # tree quality: the moved tenth, refitted, against a fresh build of the same buffers
        r.set_camera(cam0)
        r.update_primitives(first, rec_a)
        r.build_accel("lbvh")
        r.update_primitives(first, rec_b)
        r.refit_accel()
        q = r.accel_quality()
        res["q_built"], res["q_refit"] = q["q_built"], q["q_now"]
        res["q_ratio"] = round(q["q_now"] / q["q_built"], 4)

        def steps_ms():
            r.reset()
            r.frame(spp).sync()
            t = time.perf_counter()
            for _ in range(steps):
                r.frame(spp)
            r.sync()
            return round((time.perf_counter() - t) * 1e3 / steps, 3)

        res["step_ms_refit"] = steps_ms()
        r.build_accel("lbvh")
        res["step_ms_fresh"] = steps_ms()
        res["q_fresh"] = r.accel_quality()["q_now"]
        res["q_ratio_fresh"] = round(res["q_refit"] / res["q_fresh"], 4)
        res["step_ratio"] = round(res["step_ms_refit"] / res["step_ms_fresh"], 4)
        r.build_accel("ploc")
        res["step_ms_fresh_ploc"] = steps_ms()
        res["edit_total_ms"] = {"refit": round(res["refit_ms"] + res["step_ms_refit"], 3),
                                "rebuild_lbvh": round(res["build_lbvh_ms"] + res["step_ms_fresh"], 3),
                                "rebuild_ploc": round(res["build_ploc_ms"] + res["step_ms_fresh_ploc"], 3)}
        res["spp_per_step"] = spp
    finally:
        r.close()
    return res


def upload_build(ps, cnt, reps):
    """crt_upload_scene + crt_build_accel(LBVH) of the scene without its last `cnt` primitives and of the whole scene."""
    from computeraytracer_amd.scene import PackedScene
    n = len(ps.primitives)
    out = []
    with Renderer(0) as r:
        for m in (n - cnt, n):
            part = PackedScene(ps.primitives[:m], ps.lights, ps.camera, ps.spectra, ps.cie)
            out.append(timed(lambda: r.upload(part).build_accel("lbvh"), reps, warm=1))
    return out


def run_topology(name, ps, reps, upload_only=False):
    import ctypes as C
    n = len(ps.primitives)
    cnt = n // 10
    res = {"scene": name, "primitives": n, "edited": cnt, "reps": reps, "upload_build_ms": upload_build(ps, cnt, reps)}
    if upload_only:
        return res
    tail = np.ascontiguousarray(ps.primitives[n - cnt:])
    one = np.array([[n - cnt, cnt]], np.uint32)
    bounds = np.linspace(n - cnt, n, 1001).astype(np.int64)
    many = np.ascontiguousarray(np.stack([bounds[:-1], bounds[1:] - bounds[:-1]], 1).astype(np.uint32))
    with Renderer(0) as r:
        lib, h = r._lib, r._h
        r.upload(ps).build_accel("lbvh")

        def cycle(ranges, grow=False):
            """remove, rebuild, append, rebuild: the four times of one round"""
            t = [time.perf_counter()]
            r._chk(lib.crt_remove_primitives(h, ranges.ctypes.data, len(ranges), None, 0)); t.append(time.perf_counter())
            rebuilt = C.c_int()
            r._chk(lib.crt_refit_accel(h, C.byref(rebuilt))); t.append(time.perf_counter())
            assert rebuilt.value == 1
            if grow:                                              # an array without room: the cut scene uploaded afresh
                from computeraytracer_amd.scene import PackedScene
                r.upload(PackedScene(ps.primitives[:n - cnt], ps.lights, ps.camera, ps.spectra, ps.cie)).build_accel("lbvh")
                t[-1] = time.perf_counter()
            r._chk(lib.crt_append_primitives(h, tail.ctypes.data, cnt, None, 0)); t.append(time.perf_counter())
            r._chk(lib.crt_refit_accel(h, C.byref(rebuilt))); t.append(time.perf_counter())
            assert rebuilt.value == 1
            return [(b - a) * 1e3 for a, b in zip(t[:-1], t[1:])]

        def med(rows, k):
            return round(statistics.median(row[k] for row in rows), 4)

        cycle(one)
        a = [cycle(one) for _ in range(reps)]
        b = [cycle(many) for _ in range(reps)]
        g = [cycle(one, grow=True) for _ in range(max(3, reps // 4))]
        r.scene = ps                                              # (the raw calls above kept the Renderer's host copy out of it)
        assert r.read_primitives(n - 2, 2).tobytes() == ps.primitives[n - 2:].tobytes()
        from computeraytracer_amd.scene import PackedScene
        mid = np.array([[n // 3, cnt]], np.uint32)
        ts = []
        for _ in range(max(3, reps // 4)):
            r.upload(PackedScene(ps.primitives, ps.lights, ps.camera, ps.spectra, ps.cie)).build_accel("lbvh")
            t = time.perf_counter()
            r._chk(lib.crt_remove_primitives(h, mid.ctypes.data, 1, None, 0))
            ts.append((time.perf_counter() - t) * 1e3)
        res["remove_mid_ms"] = round(statistics.median(ts), 4)
        res.update(remove_one_ms=med(a, 0), rebuild_after_remove_ms=med(a, 1), append_ms=med(a, 2), rebuild_after_append_ms=med(a, 3),
                   remove_1000_ms=med(b, 0), append_grow_ms=med(g, 2))
        res["edit_rebuild_ms"] = {"remove_one": round(res["remove_one_ms"] + res["rebuild_after_remove_ms"], 4),
                                  "remove_1000": round(res["remove_1000_ms"] + med(b, 1), 4),
                                  "remove_mid": round(res["remove_mid_ms"] + res["rebuild_after_remove_ms"], 4),
                                  "append": round(res["append_ms"] + res["rebuild_after_append_ms"], 4),
                                  "append_grow": round(res["append_grow_ms"] + med(g, 3), 4)}
    return res


def policy_loop(soup_tris):
    for name, ps in [("s2", atrium250k(1920, 1080))] + ([("soup", soup(soup_tris, 1920, 1080))] if soup_tris else []):
        n = len(ps.primitives)
        first, cnt = n // 3, n // 10
        with Renderer(0) as r:
            r.upload(ps).build_accel("lbvh")
            r.set_option("refit_rebuild_pct", 100000)
            for _ in range(10):
                r.update_primitives(first, ps.primitives[first:first + cnt])
                assert not r.refit_accel()
            print(json.dumps({"scene": name, "accel": r.accel_stats(), "quality": r.accel_quality()["now"]}), flush=True)


def kernel_stats(db_path, out):
    import csv
    import sqlite3
    db = sqlite3.connect(db_path)
    groups, nodes_grid = {}, 0
    for name, grid, ns in db.execute("select name, grid_x, end - start from kernels where name like '%k_quality_%' or name like '%k_refit_quant4%' order by start"):
        if "k_quality_nodes" in name:
            nodes_grid = grid
        if "k_quality_sum" in name:
            grid = nodes_grid                                     # one block always: listed under the grid of the launch whose pairs it adds
        groups.setdefault((name, grid), []).append(ns / 1e3)
    with (open(out, "w", newline="") if out else sys.stdout) as f:
        w = csv.writer(f)
        w.writerow(["kernel", "grid_threads", "calls", "avg_us", "min_us", "max_us"])
        for (name, grid), us in sorted(groups.items()):
            w.writerow([name, grid, len(us), round(statistics.mean(us), 3), round(min(us), 3), round(max(us), 3)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--soup-tris", type=int, default=10_000_000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None, metavar="DIR", help="a built checkout of the parent commit: its update_ms, before and after")
    ap.add_argument("--update-only", action="store_true", help="build_lbvh_ms, update_ms and refit_ms only")
    ap.add_argument("--tree", default=None, metavar="DIR", help="import the package from this checkout instead of the tool's own")
    ap.add_argument("--topology", action="store_true", help="crt_remove_primitives / crt_append_primitives and the rebuilding refit instead")
    ap.add_argument("--upload-only", action="store_true", help="with --topology: upload_build_ms only (what --parent runs)")
    ap.add_argument("--policy-loop", action="store_true", help="only the refits with the policy on and one crt_accel_quality: the run to put under rocprofv3")
    ap.add_argument("--kernel-stats", default=None, metavar="DB", help="reduce that run's rocprofv3 database to the CSV (--out, or stdout)")
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.out)
    if a.policy_loop:
        return policy_loop(a.soup_tris)

    def parent_update():
        import subprocess
        mode = ["--topology", "--upload-only"] if a.topology else ["--update-only"]
        cmd = [sys.executable, os.path.abspath(__file__), *mode, "--tree", a.parent, "--reps", str(a.reps), "--soup-tris", str(a.soup_tris)]
        return json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1])

    before = parent_update() if a.parent else None
    if a.topology:
        out = {"s2": run_topology("S2 atrium250k", atrium250k(1920, 1080), a.reps, a.upload_only)}
        if a.soup_tris:
            out["soup"] = run_topology(f"soup {a.soup_tris}", soup(a.soup_tris, 1920, 1080), a.reps, a.upload_only)
        if a.parent:
            after = parent_update()
            for k in out:
                pb = out[k]["parent_upload_build_ms"] = [before[k]["upload_build_ms"], after[k]["upload_build_ms"]]
                slow = [min(pb[0][i], pb[1][i]) for i in (0, 1)]         # [without the tenth, with it]: the faster run of each
                e = out[k]["edit_rebuild_ms"]
                out[k]["ratio"] = {"remove_one": round(e["remove_one"] / slow[0], 4), "remove_1000": round(e["remove_1000"] / slow[0], 4),
                                   "remove_mid": round(e["remove_mid"] / slow[0], 4),
                                   "append": round(e["append"] / slow[1], 4), "append_grow": round(e["append_grow"] / slow[1], 4)}
        line = json.dumps(out)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    out = {"s2": run_scene("S2 atrium250k", atrium250k(1920, 1080), a.reps, a.spp, a.steps, a.update_only)}
    if a.soup_tris:
        out["soup"] = run_scene(f"soup {a.soup_tris}", soup(a.soup_tris, 1920, 1080), a.reps, a.spp, a.steps, a.update_only)
    if a.parent:
        after = parent_update()
        for k in out:
            out[k]["parent_update_ms"] = [before[k]["update_ms"], after[k]["update_ms"]]
            out[k]["parent_refit_ms"] = [before[k]["refit_ms"], after[k]["refit_ms"]]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
