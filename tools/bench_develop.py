#!/usr/bin/env python3
"""Times the way from three f64 film accumulators on the GPU to a picture on the host, the old way and the new one, at the two full-size films:
cornell (1440 x 1440, P = 3 planes) and the polarimetric room (1920 x 1088, P = 12).

  parent path   synchronise, copy the three f64 films to the host, wtgpu_develop (one host thread), imageio.tonemap (numpy)
  new path      Scene.tonemap_device to 8-bit RGBA (one kernel: k_develop_tonemap), copy the picture to the host

The two are alternated after a warm-up and the median of --reps (>= 15) is reported; the kernel's own time (device events) is reported apart from
the copy.  Also the two A/B choices of csrc/kernels_develop.hip, alternated the same way: k_develop with one lane per plane element or per pixel
(WTGPU_DEVELOP_PER_PIXEL), k_develop_tonemap with the colour table read through the caches or staged in LDS (WTGPU_TONEMAP_LDS_TABLE); the
variants' outputs are compared bit for bit.  Films are seeded random numbers: the time does not depend on their content.
Prints one JSON line; --out also writes it to a file.  Needs a GPU.  Not part of bench.py."""
import argparse
import os
import time

from film_bench_util import FILMS, alternate, event_ms, finish, need_gpu


def _scene(name, kw, env=None):
    """An uploaded scene whose knobs were read with `env` set (the knobs are read once per upload)."""
    from wave_tracer_amd import Scene
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        return Scene(name, **kw).upload(0, 65536)     # a small batch: nothing is rendered here
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def bench_film(label, reps):
    import torch
    from wave_tracer_amd import develop, imageio
    name, kw = FILMS[label]
    sc = _scene(name, kw)
    dev = torch.device("cuda", 0)
    H, W, P, stokes = sc.height, sc.width, sc.channels, sc.stokes
    g = torch.Generator(device=dev).manual_seed(1)
    value = torch.rand((H, W, P), dtype=torch.float64, device=dev, generator=g) * 30
    weight = torch.rand((H, W), dtype=torch.float64, device=dev, generator=g) * 40 + 1
    light = torch.rand((H, W, P), dtype=torch.float64, device=dev, generator=g) * 0.1
    mask = torch.rand((H, W), dtype=torch.float32, device=dev, generator=g)
    spe, tm = 16, {"op": "sRGB", "mode": "normal"}

    def parent():
        t0 = time.perf_counter()
        torch.cuda.synchronize(dev)
        v, w, l = (t.cpu().numpy() for t in (value, weight, light))
        t1 = time.perf_counter()
        img = develop(sc, v, w, l, spe)
        t2 = time.perf_counter()
        img = img.reshape(H, W, -1, stokes)[..., 0]
        imageio.tonemap(img, op="sRGB", mode="normal")
        t3 = time.perf_counter()
        return {"total_ms": (t3 - t0) * 1e3, "copy_ms": (t1 - t0) * 1e3, "develop_ms": (t2 - t1) * 1e3, "tonemap_ms": (t3 - t2) * 1e3}

    def new():
        t0 = time.perf_counter()
        k_ms, pic = event_ms(lambda: sc.tonemap_device(value, weight, light, spe, tm, 0, mask=mask, fmt="u8"))
        t1 = time.perf_counter()
        pic.cpu()
        t2 = time.perf_counter()
        # launch_and_wait_ms: the host's view of the same kernel (allocation of the result, launch, wait); after the parent path's ~100 ms on the
        # host the GPU has gone idle, and waking it is part of this figure and of kernel_ms
        return {"total_ms": (t2 - t0) * 1e3, "launch_and_wait_ms": (t1 - t0) * 1e3, "kernel_ms": k_ms, "copy_ms": (t2 - t1) * 1e3}

    out = {"film": [W, H, P], "bytes_f64_films": int(8 * (2 * value.numel() + weight.numel())), "bytes_rgba8": H * W * 4}
    out.update(alternate({"parent": parent, "new": new}, reps))
    out["new_back_to_back"] = alternate({"new": new}, reps)["new"]     # the new path alone, the GPU kept busy
    # the films are read once: value and light whole (their lines are fetched whole whichever Stokes component is wanted), the weights, the mask
    moved = out["bytes_f64_films"] + 4 * H * W + out["bytes_rgba8"]
    out["new"]["kernel_GBps"] = moved / out["new"]["kernel_ms"] / 1e6

    # A/B 1: k_develop's lane mapping
    per_pixel = _scene(name, kw, {"WTGPU_DEVELOP_PER_PIXEL": "1"})
    a, b = sc.develop_device(value, weight, light, spe), per_pixel.develop_device(value, weight, light, spe)
    torch.cuda.synchronize(dev)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the two k_develop mappings differ"
    del a, b
    out["k_develop_ms"] = alternate({"lane_per_plane": lambda: event_ms(lambda: sc.develop_device(value, weight, light, spe))[0],
                                      "lane_per_pixel": lambda: event_ms(lambda: per_pixel.develop_device(value, weight, light, spe))[0]}, reps)
    # A/B 2: the colour table of k_develop_tonemap (colourmap mode: every pixel goes through the 256-entry table)
    lds = _scene(name, kw, {"WTGPU_TONEMAP_LDS_TABLE": "1"})
    tm_cm = {"op": "sRGB", "mode": "colourmap", "table": imageio.colour_table("turbo")}
    call = lambda s: s.tonemap_device(value, weight, light, spe, tm_cm, 0, mask=mask, fmt="u8")
    a, b = call(sc), call(lds)
    torch.cuda.synchronize(dev)
    assert torch.equal(a, b), "the two table placements differ"
    del a, b
    out["k_develop_tonemap_colourmap_ms"] = alternate({"table_through_caches": lambda: event_ms(lambda: call(sc))[0],
                                                        "table_in_lds": lambda: event_ms(lambda: call(lds))[0]}, reps)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--films", default=",".join(FILMS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    need_gpu("bench_develop")
    res = {"tool": "bench_develop", "reps": max(15, args.reps), "films": {f: bench_film(f, max(15, args.reps)) for f in args.films.split(",")}}
    finish(res, args.out)


if __name__ == "__main__":
    main()
