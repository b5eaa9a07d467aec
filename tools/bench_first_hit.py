#!/usr/bin/env python3
"""Times the first-hit maps of a sensor (Scene.first_hit: depth, position, normals, uv, facing, shape and triangle ids per pixel) beside the
sensor mask (Scene.sensor_mask), which traces the same rays — the same `samples` (32) and seed — and keeps one bit of every hit.  What the
maps cost beyond the mask is the surface record of every hit and the stores.

  mask            Scene.sensor_mask, no shape flagged: the yardstick
  all_maps        every float map (14 floats per pixel) and both ids
  depth_and_ids   depth, shape and triangle: the kernel that builds no surface record
  centre_all_maps every map and both ids with one ray through the pixel's centre (samples = 0: one lane per pixel in either form)
  *_per_pixel     the first two with one lane per pixel (WTGPU_FIRST_HIT_PER_SAMPLE=0) in place of one lane per sample (the A/B of the two forms)

Scenes: cornell_box at 1440 x 1440 with full tessellation (283 K triangles), and the radio overview of tests/test_sensor_mask.py at 1440 x 1080.
Every call is timed between two device events; the calls are alternated after a warm-up and the median of --reps (>= 15) is reported, with
the quotients over the mask — reported, not judged.  Prints one JSON line; --out also writes it to a file.  Needs a GPU.  Not part of bench.py."""
import argparse
import os
import sys
import tempfile

from film_bench_util import alternate, event_ms, finish, need_gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

SAMPLES, SEED = 32, 1


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
    from test_sensor_mask import masked_radio_xml
    from wave_tracer_amd import Scene
    box = lambda: Scene("cornell_box", res=1440, mesh_detail=1, lut=(32, 32))
    yield "cornell_box_1440_full_tessellation", _upload(box, "1"), _upload(box, "0")
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "radio.xml")
        with open(f, "w") as out:
            out.write(masked_radio_xml())
        radio = lambda: Scene.from_xml(f, defines={"masked_overview": "true"}, res=1440)
        yield "radio_overview_1440", _upload(radio, "1"), _upload(radio, "0")


def bench_scene(sc, other, reps):
    import numpy as np
    import torch
    flags = np.zeros(sc.info.n_shapes)
    ms = lambda fn: (lambda: event_ms(fn)[0])
    calls = {"mask": ms(lambda: sc.sensor_mask(SAMPLES, SEED, flags)),
             "all_maps": ms(lambda: sc.first_hit(SAMPLES, SEED)),
             "depth_and_ids": ms(lambda: sc.first_hit(SAMPLES, SEED, maps=("depth",))),
             "centre_all_maps": ms(lambda: sc.first_hit(0, SEED)),
             "all_maps_per_pixel": ms(lambda: other.first_hit(SAMPLES, SEED)),
             "depth_and_ids_per_pixel": ms(lambda: other.first_hit(SAMPLES, SEED, maps=("depth",)))}
    x, y = sc.first_hit(SAMPLES, SEED), other.first_hit(SAMPLES, SEED)
    assert all(torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)) for k in x), "the two forms differ"
    del x, y
    med = alternate(calls, reps)
    # the same rays: the mask's count of hits is the maps' coverage
    cov = sc.first_hit(SAMPLES, SEED, maps=("coverage",), ids=())["coverage"]
    same_rays = bool(((sc.sensor_mask(SAMPLES, SEED, flags) > 0) == (cov > 0)).all().item())
    return {"film": [sc.width, sc.height], "triangles": int(sc.info.n_tris), "samples": SAMPLES, "ms": med, "same_pixels_hit_as_the_mask": same_rays,
            "over_mask": {k: med[k] / med["mask"] for k in med if k != "mask"}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    need_gpu("bench_first_hit")
    reps = max(15, args.reps)
    res = {"tool": "bench_first_hit", "reps": reps, "scenes": {name: bench_scene(sc, other, reps) for name, sc, other in _scenes()}}
    finish(res, args.out)
    if not all(s["same_pixels_hit_as_the_mask"] for s in res["scenes"].values()):
        sys.exit("the maps and the mask disagree on which pixels are hit")


if __name__ == "__main__":
    main()
