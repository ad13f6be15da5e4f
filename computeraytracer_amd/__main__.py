"""python -m computeraytracer_amd [--scene file.json] [--width W --height H] [--spp N] [--out image.png] [--denoise K] [--orbit N [--temporal [--variance] [--animate | --animate-device [--rebuild-pct P] | --blink P]]]
                                [--adaptive THRESHOLD [--adaptive-filtered] [--adaptive-step N] [--counts-out counts.png]]
                                [--alpha] [--aov-out PREFIX] [--matte-out PREFIX [--matte-source primitive|object|material] [--matte-slots K]]
                                [--pick X,Y] [--panorama WxH [--panorama-eye x,y,z]]
--adaptive goes with --orbit: every frame is sampled adaptively up to --spp, and with --denoise K --temporal [--variance] the
temporal filters blend it with each pixel's own tile count (option "adaptive_temporal")."""
import argparse
import json
import os
import time

from . import Renderer, image, scene


def parse_args(argv=None):
    """The command line, checked: argparse's namespace, or its error exit (status 2) for a combination that does not go."""
    ap = argparse.ArgumentParser(prog="computeraytracer_amd")
    ap.add_argument("--scene", default=None, help="scene JSON in the reference's schema (default: the cornell box)")
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--accel", default="bvh2", choices=["bvh2", "lbvh", "ploc", "none"])
    ap.add_argument("--out", default="render.png")
    ap.add_argument("--checkpoint", default=None, help="resume from / save to this .npz")
    ap.add_argument("--denoise", type=int, default=None, metavar="K",
                    help="write the image denoised with K a-trous iterations instead of the plain average (crt_denoise; with "
                         "--adaptive the variance-guided crt_denoise_adaptive)")
    ap.add_argument("--orbit", type=int, default=None, metavar="N",
                    help="N frames of --spp each with the eye turned about the look-at point (one upload and build, then "
                         "set_camera per frame), written as OUT_000.png, OUT_001.png, ...")
    ap.add_argument("--temporal", action="store_true",
                    help="with --orbit and --denoise K: frame k draws samples k * spp + 1 .. (set_sample_offset) and is blended "
                         "with the reprojected result of frame k - 1 before the filter (crt_denoise_temporal)")
    ap.add_argument("--variance", action="store_true",
                    help="with --orbit N --denoise K --temporal: the passes after the blend are variance-guided, the variance "
                         "taken from the spread of the frame means (crt_denoise_svgf)")
    ap.add_argument("--spatial", type=int, nargs="?", const=400, default=None, metavar="PCT",
                    help="with --orbit N --denoise K --temporal --variance: option svgf_spatial_pct = PCT (25..10000, 400 when "
                         "given bare): a pixel with too short a history for a temporal variance takes one from the spread of "
                         "its 7x7 neighbourhood, times PCT / 100")
    ap.add_argument("--clip", type=int, nargs="?", const=100, default=None, metavar="PCT",
                    help="with --orbit N --denoise K --temporal: option temporal_clip_pct = PCT (25..10000, 100 when given "
                         "bare): the reprojected history of a pixel is clamped to the mean +- PCT / 100 standard deviations of "
                         "the frame's own colours over its 7x7 neighbourhood.  It is for lighting that changes on surfaces that "
                         "do not (the shadows --animate drags over the floor, a light that is switched): under a fixed camera "
                         "with fixed lighting it costs some of the history's benefit")
    ap.add_argument("--animate", action="store_true",
                    help="with --orbit N --denoise K --temporal: before frame k every sphere is moved to its frame-0 centre plus "
                         "(0, 0.5 radius sin(2 pi k / 16), 0) (update_primitives + refit_accel), and option temporal_motion keeps "
                         "the history across those edits")
    ap.add_argument("--animate-device", action="store_true",
                    help="with --orbit N --denoise K --temporal: --animate's motion without uploading records: before frame "
                         "k > 0 one transform_primitives call translates every sphere by (0, up(k) - up(k - 1), 0) on the device, "
                         "up(k) = 0.5 radius sin(2 pi k / 16) in float32 with the radius of frame 0 (then refit_accel)")
    ap.add_argument("--rebuild-pct", type=int, default=None, metavar="P",
                    help="with --animate-device: option refit_rebuild_pct = P (100..100000): refit_accel rebuilds the tree once its "
                         "surface-area cost has passed P percent of what it was when built (accel_quality); the refits and the "
                         "rebuilds are printed at the end")
    ap.add_argument("--blink", type=int, default=None, metavar="P",
                    help="with --orbit N --denoise K --temporal (not with --animate / --animate-device): before every frame "
                         "k > 0 with k %% P == 0 the run of spheres that ends the scene is removed on the device if it is there, "
                         "else appended back (remove_primitives / append_primitives, then refit_accel); option temporal_motion "
                         "keeps the history across those edits")
    ap.add_argument("--adaptive", type=float, default=None, metavar="THRESHOLD",
                    help="adaptive sampling (crt_trace_adaptive): rounds of --adaptive-step samples for the 8x8 tiles whose "
                         "error is above THRESHOLD, --spp samples at most, until every tile is done; with --orbit N every "
                         "frame is sampled so (frame k from sample index k * spp + 1 on with --temporal) and the mean samples "
                         "per pixel of each frame are printed")
    ap.add_argument("--adaptive-filtered", action="store_true",
                    help="with --adaptive: THRESHOLD judges the noise the variance-guided filter leaves in the tile instead of "
                         "the raw pixel error (crt_trace_adaptive_filtered; the filter runs --denoise K iterations where given, "
                         "else its default)")
    ap.add_argument("--adaptive-step", type=int, default=16, metavar="N", help="with --adaptive: samples per round (16)")
    ap.add_argument("--adaptive-min", type=int, default=None, metavar="M",
                    help="with --adaptive: a tile below M samples is sampled whatever its error (default: min(--spp, 2N))")
    ap.add_argument("--counts-out", default=None,
                    help="with --adaptive: the per-tile sample counts as a grey PNG (with --orbit: the last frame's)")
    ap.add_argument("--alpha", action="store_true",
                    help="the PNG's alpha channel is the coverage of each pixel: the share of its camera rays that hit "
                         "something, floor(alpha * 255 + 0.5) (crt_render_aovs over the samples the image holds; also with "
                         "--adaptive, not with --orbit)")
    ap.add_argument("--aov-out", default=None, metavar="PREFIX",
                    help="the feature planes of the samples the image holds (crt_render_aovs): PREFIX_albedo.png, "
                         "PREFIX_normal.png (n * 0.5 + 0.5) and PREFIX_depth.npy (also with --adaptive, not with --orbit)")
    ap.add_argument("--matte-out", default=None, metavar="PREFIX",
                    help="the id mattes of the samples the image holds (crt_render_mattes): PREFIX_ids.npy, PREFIX_counts.npy, "
                         "PREFIX_overflow.npy and PREFIX_preview.png, the rank-0 id in false colour scaled by its coverage "
                         "(also with --adaptive, not with --orbit)")
    ap.add_argument("--matte-source", default="object", choices=("primitive", "object", "material"),
                    help="with --matte-out: what an id is (default object: one per patch, sphere and mesh)")
    ap.add_argument("--matte-slots", type=int, default=8, metavar="K",
                    help="with --matte-out: ids kept per pixel, 1..16 (default 8); PREFIX_overflow.npy counts the hits left out")
    ap.add_argument("--pick", default=None, metavar="X,Y",
                    help="after the render, what lies under pixel (X, Y) of the image (crt_pick): its primitive, object id, t, "
                         "position and normal go into the JSON line as \"pick\" (null where the pixel's ray hits nothing; not "
                         "with --orbit)")
    ap.add_argument("--panorama", default=None, metavar="WxH",
                    help="after the render, a W x H equirectangular image of the scene around --panorama-eye at --spp samples "
                         "per ray (crt_radiance_rays), written beside --out as <stem>_pano.png; its size goes into the JSON "
                         "line as \"panorama\" (not with --orbit)")
    ap.add_argument("--panorama-eye", default=None, metavar="x,y,z", help="with --panorama: the view point (default: the camera's eye)")
    args = ap.parse_args(argv)
    if args.panorama is not None:
        try:
            w, h = (int(v) for v in args.panorama.lower().split("x"))
            if w < 1 or h < 1:
                raise ValueError
        except ValueError:
            ap.error("--panorama takes WxH: two positive integers")
        args.panorama = (w, h)
        if args.orbit is not None:
            ap.error("--panorama does not go with --orbit")
    if args.panorama_eye is not None:
        try:
            eye = tuple(float(v) for v in args.panorama_eye.split(","))
            if len(eye) != 3 or args.panorama is None:
                raise ValueError
        except ValueError:
            ap.error("--panorama-eye takes x,y,z and goes with --panorama")
        args.panorama_eye = eye
    if args.pick is not None:
        try:
            x, y = (int(v) for v in args.pick.split(","))
            if x < 0 or y < 0:
                raise ValueError
        except ValueError:
            ap.error("--pick takes X,Y: two non-negative integers")
        args.pick = (x, y)
        if args.orbit is not None:
            ap.error("--pick does not go with --orbit")
    if args.matte_out and args.orbit is not None:
        ap.error("--matte-out does not go with --orbit")
    if not 1 <= args.matte_slots <= 16:
        ap.error("--matte-slots must be 1..16")
    if (args.alpha or args.aov_out) and args.orbit is not None:
        ap.error("--alpha and --aov-out do not go with --orbit")
    if args.alpha and args.out.endswith(".ppm"):
        ap.error("--alpha needs a PNG: a PPM has no alpha channel")
    if args.orbit is not None and (args.orbit < 1 or args.checkpoint):
        ap.error("--orbit needs N >= 1 and no --checkpoint")
    if args.temporal and (args.orbit is None or args.denoise is None):
        ap.error("--temporal goes with --orbit N --denoise K")
    if args.variance and not args.temporal:
        ap.error("--variance goes with --orbit N --denoise K --temporal")
    if args.spatial is not None and (not args.variance or not 25 <= args.spatial <= 10000):
        ap.error("--spatial [PCT] goes with --orbit N --denoise K --temporal --variance, PCT in 25..10000")
    if args.clip is not None and (not args.temporal or not 25 <= args.clip <= 10000):
        ap.error("--clip [PCT] goes with --orbit N --denoise K --temporal, PCT in 25..10000")
    if args.animate and not args.temporal:
        ap.error("--animate goes with --orbit N --denoise K --temporal")
    if args.animate_device and (not args.temporal or args.animate):
        ap.error("--animate-device goes with --orbit N --denoise K --temporal, and not with --animate")
    if args.rebuild_pct is not None and not args.animate_device:
        ap.error("--rebuild-pct goes with --animate-device")
    if args.blink is not None and (not args.temporal or args.animate or args.animate_device or args.blink < 1):
        ap.error("--blink P goes with --orbit N --denoise K --temporal, P >= 1, and not with --animate or --animate-device")
    if args.adaptive is not None and args.checkpoint:
        ap.error("--adaptive does not go with --checkpoint")
    if (args.counts_out or args.adaptive_min is not None) and args.adaptive is None:
        ap.error("--counts-out and --adaptive-min need --adaptive")
    if args.adaptive_filtered and args.adaptive is None:
        ap.error("--adaptive-filtered needs --adaptive")
    return args


def main(argv=None):
    args = parse_args(argv)
    sc = scene.load_scene(args.scene)
    if args.width:
        sc["camera"]["width"], sc["camera"]["height"] = args.width, args.height or args.width
    ps = scene.pack_scene(sc, base_dir=os.path.dirname(os.path.abspath(args.scene)) if args.scene else None)
    with Renderer(0) as r:
        r.upload(ps).build_accel(args.accel)
        if args.orbit is not None:
            base, ext = os.path.splitext(args.out)
            outs, t0 = [], time.time()
            if args.animate or args.animate_device:
                import math
                import numpy as np
                r.set_option("temporal_motion", 1)
                spheres = [int(i) for i in (ps.primitives["category"] == scene.CATEGORY["sphere"]).nonzero()[0]]
            if args.blink is not None:
                run = _closing_spheres(ps)
                if not 0 < run < len(ps.primitives):
                    raise SystemExit("--blink: the scene must end in a run of spheres, with a primitive before it")
                r.set_option("temporal_motion", 1)
                blink_first, blink_tail, edits = len(ps.primitives) - run, ps.primitives[len(ps.primitives) - run:], 0
            refits, mean_samples = 0, []
            if args.adaptive is not None and args.temporal:
                r.set_option("adaptive_temporal", 1)
            if args.rebuild_pct is not None:
                r.set_option("refit_rebuild_pct", args.rebuild_pct)
            if args.spatial is not None:
                r.set_option("svgf_spatial_pct", args.spatial)
            if args.clip is not None:
                r.set_option("temporal_clip_pct", args.clip)
            for k, cam in enumerate(scene.orbit_cameras(ps.camera, args.orbit)):
                if args.animate:
                    for i in spheres:
                        rec = ps.primitives[i:i + 1]
                        up = 0.5 * float(rec["data2"][0, 0]) * math.sin(2.0 * math.pi * k / 16.0)
                        r.update_primitives(i, scene.transform_records(rec, [[1, 0, 0], [0, 1, 0], [0, 0, 1]], (0.0, up, 0.0)))
                    r.refit_accel()
                if args.animate_device and k:
                    ops = []
                    for i in spheres:
                        rad = float(ps.primitives["data2"][i, 0])
                        up0, up1 = (np.float32(0.5 * rad * math.sin(2.0 * math.pi * j / 16.0)) for j in (k - 1, k))
                        ops.append((i, 1, [1, 0, 0, 0, 0, 1, 0, np.float32(up1 - up0), 0, 0, 1, 0]))
                    r.transform_primitives(ops).refit_accel()
                    refits += 1
                if args.blink is not None and k and k % args.blink == 0:
                    if len(r.scene.primitives) > blink_first:
                        r.remove_primitives([(blink_first, len(blink_tail))])
                    else:
                        r.append_primitives(blink_tail)
                    r.refit_accel()
                    edits += 1
                r.set_camera(cam)
                if args.temporal:
                    r.set_sample_offset(k * args.spp)
                if args.adaptive is not None:
                    # few samples per frame, placed where the noise is, accumulated over time (option "adaptive_temporal")
                    counts = _adaptive_rounds(r, args)[0]
                    mean_samples.append(round(_pixel_samples(counts, ps) / (ps.width * ps.height), 4))
                else:
                    r.frame(args.spp).sync()
                if args.temporal:
                    rgba = r.denoise_svgf(args.denoise) if args.variance else r.denoise_temporal(args.denoise)
                elif args.adaptive is not None:
                    rgba = r.read_rgba8() if args.denoise is None else r.denoise_adaptive(args.denoise)
                else:
                    rgba = r.read_rgba8() if args.denoise is None else r.denoise(args.denoise)
                outs.append(f"{base}_{k:03d}{ext}")
                (image.write_ppm if ext == ".ppm" else image.write_png)(outs[-1], rgba)
            info = {"width": ps.width, "height": ps.height, "frames": args.orbit, "spp": args.spp,
                    "seconds": round(time.time() - t0, 4), "out": outs}
            if args.adaptive is not None:
                info["adaptive"] = args.adaptive
                info["mean_samples"] = mean_samples               # per frame: samples per pixel
                if args.counts_out:
                    _write_counts(args.counts_out, counts, ps, args.spp)
                    info["counts_out"] = args.counts_out
            if args.denoise is not None:
                info["denoise"] = args.denoise
            if args.temporal:
                info["temporal"] = True
            if args.variance:
                info["variance"] = True
            if args.spatial is not None:
                info["spatial"] = args.spatial
            if args.animate:
                info["animate"] = True
            if args.animate_device:
                info["animate_device"] = True
            if args.blink is not None:
                info["blink"], info["edits"] = args.blink, edits
            if args.rebuild_pct is not None:
                info["rebuild_pct"] = args.rebuild_pct
                info["refits"] = refits                            # refit_accel calls, of which the policy turned ...
                info["rebuilds"] = r.accel_quality()["rebuilds"]   # ... this many into rebuilds
            print(json.dumps(info))
            return
        if args.adaptive is not None:
            _adaptive(r, ps, args)
            return
        if args.checkpoint and os.path.exists(args.checkpoint):
            image.load_checkpoint(args.checkpoint, r)
        t0 = time.time()
        r.frame(args.spp).sync()
        dt = time.time() - t0
        rgba = r.read_rgba8() if args.denoise is None else r.denoise(args.denoise)
        info = {"width": ps.width, "height": ps.height, "sample": r.sample, "seconds": round(dt, 4), "out": args.out}
        rgba = _aovs(r, args, rgba, info)
        _pick(r, args, info)
        _panorama(r, ps, args, info)
        (image.write_ppm if args.out.endswith(".ppm") else image.write_png)(args.out, rgba)
        if args.checkpoint:
            image.save_checkpoint(args.checkpoint, r)
        if args.denoise is not None:
            info["denoise"] = args.denoise
        print(json.dumps(info))


def _aovs(r, args, rgba, info):
    """--alpha, --aov-out and --matte-out: the planes of the samples the image holds; returns the rgba8 to write."""
    if args.matte_out:
        planes = r.render_mattes(0, args.matte_source, args.matte_slots)
        if args.adaptive is not None:                            # every pixel its own tile's count
            import numpy as np
            _, _, tw, th = r.tile
            n = np.repeat(np.repeat(r.read_adaptive()[0], 8, 0), 8, 1)[:th, :tw]
        else:
            n = r.sample
        info["matte_out"] = image.write_mattes(args.matte_out, planes, n)
    want = (("alpha",) if args.alpha else ()) + (("depth", "normal", "albedo") if args.aov_out else ())
    if not want:
        return rgba
    planes = r.render_aovs(0, want)
    if args.aov_out:
        info["aov_out"] = image.write_aovs(args.aov_out, planes)
    if args.alpha:
        info["alpha"] = True
        rgba = image.with_alpha(rgba, planes["alpha"])
    return rgba


def _panorama(r, ps, args, info):
    """--panorama WxH: an equirectangular view through crt_radiance_rays, <out stem>_pano.png."""
    if args.panorama is None:
        return
    w, h = args.panorama
    eye = args.panorama_eye if args.panorama_eye is not None else tuple(float(v) for v in ps.camera[0:3])
    _, rgba = r.panorama(w, h, eye, max(1, args.spp))
    path = os.path.splitext(args.out)[0] + "_pano.png"
    image.write_png(path, rgba)
    info["panorama"] = {"width": w, "height": h, "eye": list(eye), "samples": max(1, args.spp), "out": path}


def _pick(r, args, info):
    """--pick X,Y: what the pixel's camera ray hits, into the JSON line."""
    if args.pick is None:
        return
    x, y = args.pick
    w, h = r.image_size
    if x >= w or y >= h:
        raise SystemExit(f"--pick {x},{y}: outside the {w} x {h} image")
    hit = r.pick(x, y)
    info["pick"] = None if hit is None else {"x": x, "y": y, "primitive": hit["prim"], "id": hit["id"], "t": hit["t"],
                                             "position": [float(v) for v in hit["position"]],
                                             "normal": [float(v) for v in hit["normal"]]}


def _closing_spheres(ps) -> int:
    """How many spheres end the primitive list (--blink's object)."""
    cat = ps.primitives["category"]
    run = 0
    while run < len(cat) and cat[len(cat) - 1 - run] == scene.CATEGORY["sphere"]:
        run += 1
    return run


def _adaptive_rounds(r, args):
    """Rounds of --adaptive-step samples until no tile is active: (the tile counts, the rounds)."""
    rounds = 0
    min_samples = min(args.spp, 2 * args.adaptive_step) if args.adaptive_min is None else args.adaptive_min
    rule = dict(samples=args.adaptive_step, threshold=args.adaptive, min_samples=min_samples, max_samples=args.spp)
    if args.adaptive_filtered:
        trace = lambda: r.trace_adaptive_filtered(iterations=args.denoise, **rule)
    else:
        trace = lambda: r.trace_adaptive(**rule)
    while trace():
        rounds += 1
    return r.read_adaptive()[0], rounds


def _pixel_samples(counts, ps):
    import numpy as np
    return int(np.repeat(np.repeat(counts, 8, 0), 8, 1)[:ps.height, :ps.width].sum(dtype=np.uint64))


def _write_counts(path, counts, ps, spp):
    import numpy as np
    grey = (counts.astype(np.float64) * (255.0 / max(1, spp))).clip(0, 255).astype(np.uint8)
    rgba = np.repeat(np.repeat(grey, 8, 0), 8, 1)[:ps.height, :ps.width, None].repeat(4, 2)
    rgba[..., 3] = 255
    image.write_png(path, rgba)


def _adaptive(r, ps, args):
    import numpy as np
    t0 = time.time()
    counts, rounds = _adaptive_rounds(r, args)
    dt = time.time() - t0
    rgba = r.read_rgba8() if args.denoise is None else r.denoise_adaptive(args.denoise)
    info = {"width": ps.width, "height": ps.height, "adaptive": args.adaptive, "rounds": rounds,
            "pixel_samples": _pixel_samples(counts, ps), "seconds": round(dt, 4),
            "tile_samples": {"min": int(counts.min()), "median": float(np.median(counts)), "max": int(counts.max())},
            "out": args.out}
    rgba = _aovs(r, args, rgba, info)
    _pick(r, args, info)
    _panorama(r, ps, args, info)
    (image.write_ppm if args.out.endswith(".ppm") else image.write_png)(args.out, rgba)
    if args.denoise is not None:
        info["denoise"] = args.denoise
    if args.counts_out:
        _write_counts(args.counts_out, counts, ps, args.spp)
        info["counts_out"] = args.counts_out
    print(json.dumps(info))


if __name__ == "__main__":
    main()
