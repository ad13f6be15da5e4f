"""python -m computeraytracer_amd [--scene file.json] [--width W --height H] [--spp N] [--out image.png] [--denoise K] [--orbit N]"""
import argparse
import json
import os
import time

from . import Renderer, image, scene


def main():
    ap = argparse.ArgumentParser(prog="computeraytracer_amd")
    ap.add_argument("--scene", default=None, help="scene JSON in the reference's schema (default: the cornell box)")
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--accel", default="bvh2", choices=["bvh2", "lbvh", "none"])
    ap.add_argument("--out", default="render.png")
    ap.add_argument("--checkpoint", default=None, help="resume from / save to this .npz")
    ap.add_argument("--denoise", type=int, default=None, metavar="K",
                    help="write the image denoised with K a-trous iterations (crt_denoise) instead of the plain average")
    ap.add_argument("--orbit", type=int, default=None, metavar="N",
                    help="N frames of --spp each with the eye turned about the look-at point (one upload and build, then "
                         "set_camera per frame), written as OUT_000.png, OUT_001.png, ...")
    args = ap.parse_args()
    if args.orbit is not None and (args.orbit < 1 or args.checkpoint):
        ap.error("--orbit needs N >= 1 and no --checkpoint")
    sc = scene.load_scene(args.scene)
    if args.width:
        sc["camera"]["width"], sc["camera"]["height"] = args.width, args.height or args.width
    ps = scene.pack_scene(sc, base_dir=os.path.dirname(os.path.abspath(args.scene)) if args.scene else None)
    with Renderer(0) as r:
        r.upload(ps).build_accel(args.accel)
        if args.orbit is not None:
            base, ext = os.path.splitext(args.out)
            outs, t0 = [], time.time()
            for k, cam in enumerate(scene.orbit_cameras(ps.camera, args.orbit)):
                r.set_camera(cam).frame(args.spp).sync()
                rgba = r.read_rgba8() if args.denoise is None else r.denoise(args.denoise)
                outs.append(f"{base}_{k:03d}{ext}")
                (image.write_ppm if ext == ".ppm" else image.write_png)(outs[-1], rgba)
            info = {"width": ps.width, "height": ps.height, "frames": args.orbit, "spp": args.spp,
                    "seconds": round(time.time() - t0, 4), "out": outs}
            if args.denoise is not None:
                info["denoise"] = args.denoise
            print(json.dumps(info))
            return
        if args.checkpoint and os.path.exists(args.checkpoint):
            image.load_checkpoint(args.checkpoint, r)
        t0 = time.time()
        r.frame(args.spp).sync()
        dt = time.time() - t0
        rgba = r.read_rgba8() if args.denoise is None else r.denoise(args.denoise)
        (image.write_ppm if args.out.endswith(".ppm") else image.write_png)(args.out, rgba)
        if args.checkpoint:
            image.save_checkpoint(args.checkpoint, r)
        info = {"width": ps.width, "height": ps.height, "sample": r.sample, "seconds": round(dt, 4), "out": args.out}
        if args.denoise is not None:
            info["denoise"] = args.denoise
        print(json.dumps(info))


if __name__ == "__main__":
    main()
