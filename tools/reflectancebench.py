"""Developer tool: three routes from a pixel-interleaved reflectance cube to the resident normalised raster, on the same
seeded cube; the rasters are compared bit for bit before anything is timed.

    python tools/reflectancebench.py [--size 1000] [--bands 426] [--precision bf16] [--calls 20] [--host-runs 3] [--out FILE]
    DTA_DEV_LIB=1 DTA_REFLECTANCE_PIXELS=16 python tools/reflectancebench.py      # developer library: 16, 32 or 64 pixels per workgroup

  (a) today's route: np.ascontiguousarray(np.moveaxis(cube[:, :, sel], 2, 0)) on the host (`host_select_transpose_s`), then
      DenseRaster(band_first) (`denseraster_s`: upload + k_raster_normalise; the kernel alone: `raster_normalise_ms`)
  (b) DenseRaster.from_reflectance(cube) from the host cube, strips of 64 MiB (`from_host_cube_s`)
  (c) DenseRaster.from_reflectance(cube) from a device-resident cube (`from_device_cube_ms`), and its kernel alone through
      the C entry on buffers allocated once (`reflectance_normalise_ms`), with the bytes it has to move over that time

Host times: wall clock around work that ends in a device synchronise, the median of `host-runs` runs after one warm-up run.
Kernel times: stream events, the median of `calls` calls after five warm-up calls, with the minimum and the maximum.  Prints
one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deeptreeattention_amd import _lib, reflectance as R  # noqa: E402
from deeptreeattention_amd.dense import DenseRaster  # noqa: E402


def wall(fn, runs):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), times


def events(fn, calls):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(max(calls, 20)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1000)
    ap.add_argument("--bands", type=int, default=426)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "reflectancebench needs the MI355X"
    dev = torch.device("cuda:0")
    H = W = a.size
    B = a.bands
    bands = "no_water" if B >= 425 else "all"
    rng = np.random.default_rng(0)
    cube = rng.integers(-100, 10000, (H, W, B), dtype=np.int16)
    cube[rng.random((H, W)) < 0.01] = -9999
    sel_file = R.band_index(bands, B)                       # the bands of the file the reference would write
    sel = R.selected_bands(bands, B, 10)                    # the bands of the raster
    C, NC = len(sel), (len(sel) + 15) // 16
    tiles = a.precision == "bf16"

    band_first = [None]

    def host_part():
        band_first[0] = np.ascontiguousarray(np.moveaxis(cube[:, :, sel_file], 2, 0))
    host_s, host_runs = wall(host_part, a.host_runs)
    old = DenseRaster(band_first[0], clip=10, precision=a.precision, device=dev)
    new = DenseRaster.from_reflectance(cube, bands, clip=10, precision=a.precision, device=dev)
    dcube = torch.from_numpy(cube).to(dev)
    res_new = DenseRaster.from_reflectance(dcube, bands, clip=10, precision=a.precision, device=dev)
    torch.cuda.synchronize()
    assert torch.equal(old.data.view(torch.int16), new.data.view(torch.int16)), "from_reflectance (host cube) differs from DenseRaster"
    assert torch.equal(old.data.view(torch.int16), res_new.data.view(torch.int16)), "from_reflectance (device cube) differs from DenseRaster"
    del new, res_new

    old_s, _ = wall(lambda: DenseRaster(band_first[0], clip=10, precision=a.precision, device=dev), a.host_runs)
    b_s, _ = wall(lambda: DenseRaster.from_reflectance(cube, bands, clip=10, precision=a.precision, device=dev), a.host_runs)

    L = _lib.lib()
    raw = torch.from_numpy(band_first[0]).to(dev)
    out = torch.empty_like(old.data)
    st = _lib.current_stream_ptr()
    k_old = events(lambda: _lib.check(L.dta_raster_normalise(_lib.ptr(raw), len(sel_file), H, W, 10, _lib.CROP_I16, int(tiles),
                                                             _lib.ptr(out), st), "dta_raster_normalise"), a.calls)
    assert torch.equal(out.view(torch.int16), old.data.view(torch.int16))
    del raw
    index = torch.from_numpy(sel).to(dev)
    d = _lib.ReflectanceDesc(B, W, H, 0, W, _lib.CROP_I16, int(tiles), H, 0)
    out.zero_()
    k_new = events(lambda: _lib.check(L.dta_reflectance_normalise(d, _lib.ptr(dcube), _lib.ptr(index), C, _lib.ptr(out), st),
                                      "dta_reflectance_normalise"), a.calls)
    assert torch.equal(out.view(torch.int16), old.data.view(torch.int16))
    c_ms = events(lambda: DenseRaster.from_reflectance(dcube, bands, clip=10, precision=a.precision, device=dev), a.calls)

    out_bytes = NC * H * W * 32 if tiles else C * H * W * 4
    new_bytes = H * W * B * 2 + out_bytes                       # the cube once, the raster once
    old_bytes = C * H * W * 2 + out_bytes                       # the kept planes once (the second read is served by L2), the raster once
    pixels, stride = R.launch_plan(B, 2, W)
    res = {"workload": "reflectance cube -> resident raster: band mask, clip 10, per-pixel min-max, transpose",
           "cube": [H, W, B], "dtype": "int16", "bands": bands, "raster_bands": C, "precision": a.precision,
           "host_select_transpose_s": round(host_s, 3), "host_select_transpose_runs_s": [round(t, 3) for t in host_runs],
           "denseraster_s": round(old_s, 4), "route_a_total_s": round(host_s + old_s, 3),
           "from_host_cube_s": round(b_s, 4),
           "from_device_cube_ms": [round(v, 4) for v in c_ms],
           "reflectance_normalise_ms": [round(v, 4) for v in k_new], "reflectance_normalise_bytes": new_bytes,
           "reflectance_normalise_tb_per_s": round(new_bytes / (k_new[0] * 1e-3) / 1e12, 3),
           "raster_normalise_ms": [round(v, 4) for v in k_old], "raster_normalise_bytes": old_bytes,
           "raster_normalise_tb_per_s": round(old_bytes / (k_old[0] * 1e-3) / 1e12, 3),
           "kernel_time_ratio": round(k_new[0] / k_old[0], 3), "bytes_ratio": round(new_bytes / old_bytes, 3),
           "pixels_per_workgroup": pixels, "lds_pixel_stride": stride,
           "pixels_switch": os.environ.get("DTA_REFLECTANCE_PIXELS") if L.dta_dev_switches_enabled() else None,
           "ms_fields": "median, min, max", "calls": max(a.calls, 20),
           "bit_identical_to_denseraster": True, "build_id": L.dta_build_id().decode()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
