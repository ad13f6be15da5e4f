"""Readout step after the path (replaces the reference's blit pass,
TextureRenderShader.wgsl + src/main.js:612-617): rgba8 -> PPM / PNG files, and the
f32 XYZ accumulator + sample index as a resumable checkpoint (.npz)."""
from __future__ import annotations

import struct
import zlib

import numpy as np


def write_ppm(path: str, rgba: np.ndarray) -> None:
    """Binary P6, row 0 = top (same orientation as the reference's canvas)."""
    h, w = rgba.shape[:2]
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(np.ascontiguousarray(rgba[..., :3]).tobytes())


def write_png(path: str, rgba: np.ndarray) -> None:
    """8-bit RGBA PNG with the standard library only."""
    h, w = rgba.shape[:2]
    rows = np.empty((h, 1 + w * 4), np.uint8)
    rows[:, 0] = 0
    rows[:, 1:] = np.ascontiguousarray(rgba, np.uint8).reshape(h, w * 4)

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))


def unorm8(v) -> np.ndarray:
    """floor(v * 255 + 0.5) as uint8, v clamped to [0, 1] (a NaN gives 0): how a float plane goes into a PNG channel."""
    v = np.asarray(v, np.float32)
    v = np.where(v > 0, np.minimum(v, np.float32(1)), np.float32(0))
    return np.floor(v * np.float32(255) + np.float32(0.5)).astype(np.uint8)


def with_alpha(rgba: np.ndarray, alpha) -> np.ndarray:
    """A copy of rgba (H, W, 4) uint8 whose alpha channel is unorm8(alpha): the coverage plane of Renderer.render_aovs."""
    out = np.array(rgba, np.uint8)
    out[..., 3] = unorm8(alpha)
    return out


def write_aovs(prefix: str, planes: dict) -> list:
    """PREFIX_albedo.png (the albedo plane, opaque), PREFIX_normal.png (n * 0.5 + 0.5, opaque) and PREFIX_depth.npy (the
    depth plane as it is) from Renderer.render_aovs' dict; returns the paths written."""
    opaque = np.ones(planes["albedo"].shape[:2] + (1,), np.float32)
    write_png(prefix + "_albedo.png", unorm8(np.concatenate([planes["albedo"][..., :3], opaque], -1)))
    write_png(prefix + "_normal.png", unorm8(np.concatenate([planes["normal"][..., :3] * np.float32(0.5) + np.float32(0.5), opaque], -1)))
    np.save(prefix + "_depth.npy", planes["depth"])
    return [prefix + "_albedo.png", prefix + "_normal.png", prefix + "_depth.npy"]


def id_colour(ids) -> np.ndarray:
    """ids (uint32, any shape) -> (..., 3) uint8: a fixed hash of the id (the lowbias32 mixer), its three low bytes
    lifted into 64..255 so that no id is dark."""
    x = np.asarray(ids, np.uint32).astype(np.uint64)             # (64-bit products, masked back to 32 bits)
    m = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & m
    x ^= x >> np.uint64(16)
    rgb = np.stack([(x >> np.uint64(s)) & np.uint64(0xFF) for s in (0, 8, 16)], -1)
    return (np.uint64(64) + rgb * np.uint64(3) // np.uint64(4)).astype(np.uint8)


def id_preview(planes: dict, n) -> np.ndarray:
    """A false-colour view of Renderer.render_mattes' dict, (H, W, 4) uint8, opaque: id_colour of each pixel's rank-0 id
    scaled by that id's coverage count / n (n: a scalar or an (H, W) array); black where the pixel has no entry."""
    ids, counts = np.asarray(planes["ids"])[0], np.asarray(planes["counts"])[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        cov = counts.astype(np.float32) / np.asarray(n).astype(np.float32)
    rgb = id_colour(ids).astype(np.float32) / np.float32(255) * np.where(counts > 0, cov, np.float32(0))[..., None]
    return unorm8(np.concatenate([rgb, np.ones(ids.shape + (1,), np.float32)], -1))


def write_mattes(prefix: str, planes: dict, n) -> list:
    """PREFIX_ids.npy, PREFIX_counts.npy, PREFIX_overflow.npy (the planes as they are) and PREFIX_preview.png (id_preview)
    from Renderer.render_mattes' dict; returns the paths written."""
    paths = []
    for p in ("ids", "counts", "overflow"):
        np.save(f"{prefix}_{p}.npy", planes[p])
        paths.append(f"{prefix}_{p}.npy")
    write_png(prefix + "_preview.png", id_preview(planes, n))
    return paths + [prefix + "_preview.png"]


def save_checkpoint(path: str, renderer) -> None:
    """alt_color_buffer + sample: everything needed to resume."""
    np.savez_compressed(path, accum=renderer.read_accum(), sample=np.uint32(renderer.sample), tile=np.asarray(renderer.tile))


def load_checkpoint(path: str, renderer) -> int:
    d = np.load(path)
    if tuple(int(v) for v in d["tile"]) != tuple(renderer.tile):
        raise ValueError("checkpoint tile does not match the renderer's tile")
    renderer.write_accum(d["accum"], int(d["sample"]))
    return int(d["sample"])
