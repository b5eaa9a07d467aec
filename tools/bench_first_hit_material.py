#!/usr/bin/env python3
"""Times the first-hit material maps of a sensor (Scene.first_hit_material: albedo, specular reflectance, opacity, roughness and emission per
pixel and wavenumber, material index and leaf type) beside the first-hit maps that trace the same rays and build the same surface record
(Scene.first_hit with NORMAL_SHADING | UV | FACING, the same `samples` and seed): what the material maps cost beyond them is the material layer
at every hit — wrappers, textures, Fresnel — and the stores.

  first_hit           Scene.first_hit(maps = normal_shading, uv, facing; no ids): the yardstick
  all_maps            every material map at the three channel wavenumbers (15 floats per pixel) and both ids
  albedo              ALBEDO alone at one wavenumber, no ids: the kernel without the Fresnel code
  *_per_pixel         the same with one lane per pixel (WTGPU_FIRST_HIT_PER_SAMPLE=0) in place of one lane per sample (the A/B of the two forms)
  centre_*            the same three with one ray through the pixel's centre (samples = 0: one lane per pixel in either form)

Scenes: cornell_box at 1440 x 1440 with full tessellation (283 K triangles), and tests/data/xml/textured.xml variant 1 (the checker) at 1440 x 1440.
Every call is timed between two device events; the calls are alternated after a warm-up and the median of --reps (>= 15) is reported, with
the quotients over the yardstick — reported, not judged.  Prints one JSON line; --out also writes it to a file.  --kernel-only runs the
device calls alone a few times, for a kernel trace taken in a run of its own (rocprofv3 --kernel-trace --stats -- python
tools/bench_first_hit_material.py --kernel-only).  Needs a GPU.  Not part of bench.py."""
import argparse
import os
import sys

from film_bench_util import alternate, event_ms, finish, need_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES, SEED = 32, 1
YARDSTICK = ("normal_shading", "uv", "facing")


def _upload(make, per_sample):
    """An uploaded scene whose knobs were read with WTGPU_FIRST_HIT_PER_SAMPLE = per_sample (the knobs are read once per upload)."""
    old = os.environ.get("WTGPU_FIRST_HIT_PER_SAMPLE")
    os.environ["WTGPU_FIRST_HIT_PER_SAMPLE"] = per_sample
    try:
        return make().upload(0, 65536)     # a small batch: nothing is rendered here
    finally:
        os.environ.pop("WTGPU_FIRST_HIT_PER_SAMPLE") if old is None else os.environ.__setitem__("WTGPU_FIRST_HIT_PER_SAMPLE", old)


def _scenes():
    """(name, the scene with one lane per sample, the scene with one lane per pixel)"""
    from wave_tracer_amd import Scene
    box = lambda: Scene("cornell_box", res=1440, mesh_detail=1, lut=(32, 32))
    yield "cornell_box_1440_full_tessellation", _upload(box, "1"), _upload(box, "0")
    checker = lambda: Scene.from_xml(os.path.join(ROOT, "tests", "data", "xml", "textured.xml"), defines={"variant": 1}, res=1440)
    yield "textured_checker_1440", _upload(checker, "1"), _upload(checker, "0")


def _calls(sc, other):
    k = sc.channel_wavenumbers()
    full = lambda s, n: s.first_hit_material(n, SEED, k)
    albedo = lambda s, n: s.first_hit_material(n, SEED, k[:1], maps=("albedo",), ids=())
    yard = lambda s, n: s.first_hit(n, SEED, maps=YARDSTICK, ids=())
    return {"first_hit": lambda: yard(sc, SAMPLES), "all_maps": lambda: full(sc, SAMPLES), "albedo": lambda: albedo(sc, SAMPLES),
            "first_hit_per_pixel": lambda: yard(other, SAMPLES), "all_maps_per_pixel": lambda: full(other, SAMPLES),
            "albedo_per_pixel": lambda: albedo(other, SAMPLES),
            "centre_first_hit": lambda: yard(sc, 0), "centre_all_maps": lambda: full(sc, 0), "centre_albedo": lambda: albedo(sc, 0)}


def bench_scene(sc, other, reps):
    import torch
    calls = _calls(sc, other)
    x, y = calls["all_maps"](), calls["all_maps_per_pixel"]()
    torch.cuda.synchronize()
    assert all(torch.equal(x[n].view(torch.int32), y[n].view(torch.int32)) for n in x), "the two forms differ"
    del x, y
    med = alternate({n: (lambda fn=fn: event_ms(fn)[0]) for n, fn in calls.items()}, reps)
    over = {n: med[n] / med["centre_first_hit" if n.startswith("centre_") else "first_hit_per_pixel" if n.endswith("_per_pixel") else "first_hit"]
            for n in med if "first_hit" not in n}
    return {"film": [sc.width, sc.height], "triangles": int(sc.info.n_tris), "samples": SAMPLES, "n_k": 3, "ms": med, "over_first_hit": over}


def kernel_only(sc, other, calls):
    import torch
    fns = _calls(sc, other)
    for _ in range(calls):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    return {"calls_of_each": calls, "paths": sorted(fns)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    need_gpu("bench_first_hit_material")
    reps = max(15, args.reps)
    if args.kernel_only:
        res = {"tool": "bench_first_hit_material", "kernel_only": {name: kernel_only(sc, other, 5) for name, sc, other in _scenes()}}
    else:
        res = {"tool": "bench_first_hit_material", "reps": reps, "scenes": {name: bench_scene(sc, other, reps) for name, sc, other in _scenes()}}
    finish(res, args.out)


if __name__ == "__main__":
    main()
