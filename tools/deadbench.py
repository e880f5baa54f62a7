"""Developer tool: dead.RgbRaster.crops (one launch for all crowns) on a resident RGB raster vs the host route it replaces
(NumPy slicing of every padded box, then torch's CPU ToTensor / Normalize arithmetic and F.interpolate, one crown at a time),
on the same input; the device result is compared with dead.crops_np on a sample of crowns before anything is timed.

    python tools/deadbench.py [--crowns 4096] [--size 224] [--raster 2000] [--calls 20] [--write-gbs 6400] [--out FILE]

The workload: `crowns` boxes with sides of 20-80 px anywhere on a 3 x raster x raster uint8 tile (some hang over its edges),
pad 10, ImageNet normalisation.  The device time is the median of `calls` stream-event timings after a warm-up, boxes and
output buffer resident, for float32 and bfloat16 output, contiguous and channels_last.  `--write-gbs`: the streaming write
rate of the part in GB/s (tools/probe_stream.hip, run next to this tool); the bytes written divided by it is the floor the
kernel is set against.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deeptreeattention_amd import _lib, dead  # noqa: E402


def workload(crowns, raster, seed=0):
    rng = np.random.default_rng(seed)
    tile = rng.integers(0, 256, (3, raster, raster), dtype=np.uint8)
    r0 = rng.integers(-20, raster - 20, crowns)
    c0 = rng.integers(-20, raster - 20, crowns)
    boxes = np.stack([r0, c0, r0 + rng.integers(20, 81, crowns), c0 + rng.integers(20, 81, crowns)], 1).astype(np.int32)
    return tile, boxes


def host_route(tile, boxes, size, pad):
    """What a CPU worker does per crown, without the file read: slice, ToTensor, Normalize, Resize."""
    m = torch.tensor(dead.IMAGENET_MEAN).view(3, 1, 1)
    s = torch.tensor(dead.IMAGENET_STD).view(3, 1, 1)
    H, W = tile.shape[1:]
    out = torch.empty(len(boxes), 3, size, size)
    for n, (a, b, c, d) in enumerate(boxes.astype(np.int64)):
        win = tile[:, max(a - pad, 0):min(c + pad, H), max(b - pad, 0):min(d + pad, W)]
        img = (torch.from_numpy(np.ascontiguousarray(win)).float() / 255 - m) / s
        out[n] = F.interpolate(img[None], size=(size, size), mode="bilinear", align_corners=False)[0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crowns", type=int, default=4096)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--raster", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--write-gbs", type=float, default=6400.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "deadbench needs the MI355X"
    dev = torch.device("cuda:0")
    tile, boxes = workload(a.crowns, a.raster)
    pad = 10

    t0 = time.perf_counter()
    host_route(tile, boxes, a.size, pad)
    host_s = time.perf_counter() - t0

    ras = dead.RgbRaster(tile, device=dev)
    dboxes = torch.from_numpy(boxes).to(dev)
    sample = np.arange(0, a.crowns, max(1, a.crowns // 64))
    want, wvalid = dead.crops_np(tile, boxes[sample], size=a.size, pad=pad)
    res = {"workload": "dead.RgbRaster.crops: box + pad, normalise, bilinear resize, one launch", "crowns": a.crowns,
           "size": a.size, "raster": [3, a.raster, a.raster], "box_sides": [20, 80], "pad": pad, "calls": max(a.calls, 20),
           "host_route_s": round(host_s, 3), "write_rate_gbs": a.write_gbs, "groups_switch": os.environ.get("DTA_RGB_CROPS_GROUPS"),
           "dev_lib": os.environ.get("DTA_DEV_LIB") == "1"}
    for name, dtype, cl in (("fp32", torch.float32, False), ("bf16", torch.bfloat16, False),
                            ("fp32_channels_last", torch.float32, True), ("bf16_channels_last", torch.bfloat16, True)):
        fmt = torch.channels_last if cl else torch.contiguous_format
        out = torch.empty((a.crowns, 3, a.size, a.size), dtype=dtype, device=dev, memory_format=fmt)
        x, valid = ras.crops(dboxes, size=a.size, pad=pad, dtype=dtype, channels_last=cl, out=out)
        got = x[torch.from_numpy(sample).to(dev)].float().cpu().numpy()
        rel = 0.0 if dtype == torch.float32 else 2.0 ** -8
        assert bool(valid.all()) and wvalid.all()
        assert float((np.abs(got - want) - rel * np.abs(want)).max()) <= 1e-5, "device and definition disagree: " + name
        for _ in range(5):
            ras.crops(dboxes, size=a.size, pad=pad, dtype=dtype, channels_last=cl, out=out)
        torch.cuda.synchronize()
        times = []
        for _ in range(max(a.calls, 20)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ras.crops(dboxes, size=a.size, pad=pad, dtype=dtype, channels_last=cl, out=out)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        ms = float(np.median(times))
        nbytes = out.numel() * out.element_size()
        floor_ms = nbytes / (a.write_gbs * 1e9) * 1e3
        res[name] = {"device_ms_median": round(ms, 4), "device_ms_min": round(min(times), 4), "device_ms_max": round(max(times), 4),
                     "bytes_written": nbytes, "write_floor_ms": round(floor_ms, 4), "fraction_of_write_rate": round(floor_ms / ms, 3),
                     "gb_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1), "speedup_over_host": round(host_s * 1e3 / ms, 1)}
        del out, x
    res["build_id"] = _lib.lib().dta_build_id().decode()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
