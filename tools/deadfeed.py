"""Developer tool: what feeds the alive/dead classifier's training step.  One batch of 128 crops at 224 x 224 from a resident
dead.ImagePool (dta_image_pool_batch: normalise, resize, flip, labels) against RgbRaster.crops (dta_rgb_crops, the kernel the
pool's was derived from) writing the same 128 x 3 x 224 x 224 output from boxes of the same sizes in one raster -- the
yardstick: the same stores, without the per-image table and the flips -- and, on the CPU, the reference's route restated with
torch operations (PIL decode, /255, normalise, F.interpolate, flip), which train_dead.py runs on the main thread per step.

    python tools/deadfeed.py [--images DIR] [--blocks 10] [--block-calls 20] [--cpu-batches 3] [--no-gpu] [--out FILE]

The pool is shaped like the reference's training set: 5,701 images, sides 25 to 164 pixels with a median of 56 (synthetic
pixels; --images DIR takes an ImageFolder instead, for the CPU route too).  The device routes write into fixed outputs;
after a warm-up, blocks of `block-calls` launches ALTERNATE between the routes in the same call, every launch timed with a
pair of stream events read after its block; a route's figure is the median over all its launches, its spread the lowest and
highest block median, and the bytes written per second follow from the median.  The CPU route decodes JPEGs (the synthetic
images are encoded in memory first) with as many threads as torch has.  One JSON line."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deeptreeattention_amd import dead  # noqa: E402
from deeptreeattention_amd.dead import IMAGENET_MEAN, IMAGENET_STD  # noqa: E402
from deeptreeattention_amd.dead_train import IMG_EXTENSIONS  # noqa: E402

N, B, S = 5701, 128, 224


def synthetic(n, seed=0):
    rng = np.random.default_rng(seed)
    sides = np.clip(np.rint(56 * np.exp(rng.normal(0, 0.4, (n, 2)))), 25, 164).astype(int)
    return [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for h, w in sides], rng.integers(0, 2, n)


def block(fn, calls):
    ev = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def summary(blocks, written):
    per_block = [float(np.median(b)) for b in blocks]
    every = [t for b in blocks for t in b]
    ms = float(np.median(every))
    return {"ms_median": round(ms, 4), "block_median_min": round(min(per_block), 4), "block_median_max": round(max(per_block), 4),
            "calls": len(every), "bytes_written": written, "tb_written_per_s": round(written / (ms * 1e-3) / 1e12, 3)}


def device_routes(images, labels, blocks, calls):
    dev = torch.device("cuda:0")
    pool = dead.ImagePool(images, labels, device=dev)
    rng = np.random.default_rng(1)
    index = torch.from_numpy(rng.integers(0, len(pool), B)).to(dev)
    flip = torch.from_numpy((rng.random(B) < 0.5).astype(np.uint8)).to(dev)
    m, s = dead._norm(IMAGENET_MEAN, IMAGENET_STD, 3)
    # the yardstick: boxes of the batch's image sizes, laid out in one raster
    sizes = np.stack([pool.heights, pool.widths], 1)[index.cpu().numpy()]
    side = 2048
    raster = dead.RgbRaster(rng.integers(0, 256, (3, side, side), dtype=np.uint8), device=dev)
    r0, c0 = rng.integers(0, side - 164, B), rng.integers(0, side - 164, B)
    boxes = raster._boxes(np.stack([r0, c0, r0 + sizes[:, 0], c0 + sizes[:, 1]], 1).astype(np.int32))
    valid = torch.empty(B, dtype=torch.bool, device=dev)
    y = torch.empty(B, dtype=torch.int64, device=dev)
    out = {}
    for dtype, name in ((torch.float32, "float32"), (torch.bfloat16, "bfloat16")):
        x = torch.empty((B, 3, S, S), dtype=dtype, device=dev)
        routes = {"image_pool_batch": lambda: pool._launch(index, 0, B, flip, False, 0, 0, S, m, s, x, False, y),
                  "rgb_crops": lambda: raster._launch(boxes, S, 0, m, s, x, False, valid)}
        for fn in routes.values():
            block(fn, 5)
        times = {k: [] for k in routes}
        for _ in range(blocks):
            for k, fn in routes.items():
                times[k].append(block(fn, calls))
        out[name] = {k: summary(v, x.numel() * x.element_size()) for k, v in times.items()}
    out["pool"] = {"images": len(pool), "bytes": int(pool.data.numel()), "median_side": float(np.median(sizes))}
    return out


def cpu_route(jpegs, batches):
    """train_dead.py's feed for one batch, restated: decode, ToTensor, Normalize, Resize([224, 224]), RandomHorizontalFlip."""
    from PIL import Image
    mean = torch.tensor(IMAGENET_MEAN).view(3, 1, 1)
    std = torch.tensor(IMAGENET_STD).view(3, 1, 1)
    rng = np.random.default_rng(2)
    times = []
    for _ in range(batches):
        pick = rng.integers(0, len(jpegs), B)
        t0 = time.perf_counter()
        xs = []
        for i in pick:
            im = np.asarray(Image.open(io.BytesIO(jpegs[i])).convert("RGB"))
            t = (torch.from_numpy(im.copy()).permute(2, 0, 1).float() / 255 - mean) / std
            t = F.interpolate(t[None], size=(S, S), mode="bilinear", align_corners=False)[0]
            xs.append(t.flip(-1) if rng.random() < 0.5 else t)
        torch.stack(xs)
        times.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": round(float(np.median(times)), 2), "ms_min": round(min(times), 2), "ms_max": round(max(times), 2),
            "batches": batches, "threads": torch.get_num_threads()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", default=None, help="an ImageFolder (class directories of images) instead of synthetic images")
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--block-calls", type=int, default=20)
    ap.add_argument("--cpu-batches", type=int, default=3)
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"tool": "deadfeed", "batch": B, "size": S, "source": a.images or "synthetic"}
    if a.images:
        from PIL import Image
        paths = sorted(os.path.join(d, f) for d, _, fs in os.walk(a.images) for f in fs if f.lower().endswith(IMG_EXTENSIONS))
        classes = sorted(d.name for d in os.scandir(a.images) if d.is_dir())
        images = [np.asarray(Image.open(p).convert("RGB")).transpose(2, 0, 1) for p in paths]
        labels = [classes.index(os.path.relpath(p, a.images).split(os.sep)[0]) for p in paths]
        jpegs = [open(p, "rb").read() for p in paths[:4 * B]]
    else:
        images, labels = synthetic(N)
        jpegs = None
    if not a.no_gpu:
        res["device"] = device_routes(images, labels, a.blocks, a.block_calls)
        res["device_name"] = torch.cuda.get_device_name(0)
    if a.cpu_batches > 0:
        try:
            from PIL import Image
            if jpegs is None:
                jpegs = []
                for im in images[:4 * B]:
                    buf = io.BytesIO()
                    Image.fromarray(im.transpose(1, 2, 0)).save(buf, format="JPEG")
                    jpegs.append(buf.getvalue())
            res["cpu_reference_route"] = cpu_route(jpegs, a.cpu_batches)
        except ImportError:
            res["cpu_reference_route"] = "PIL is not installed"
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
