#!/usr/bin/env python3
"""Times the zonal film statistics (Scene.film_zonal_device: one pass, a record per (zone, plane)) at the two full-size films — cornell (1440 x 1440,
P = 3 planes) and the polarimetric room (1920 x 1088, P = 12) — in both forms of k_film_zonal, against two yardsticks that the same run takes:

  stats_256        one Scene.film_stats_device call with 256 bins and no mask: what ONE class costs today
  stats_2_masked   two masked film_stats_device calls, the Z = 2 question asked the old way

Zone plans: Z = 2 halves; 48 coherent blocks (shape-like); 8 x 8 cells (about 32 K zones); uniformly random labels, Z = 64 and 4096 (the worst case:
no wavefront shares a zone; 128 and 200 for tables of 41 KB and 64 KB at three planes).  Each plan without bins and with bins (256, or 32 for the cells: n_zones x bins <= 2^20), in the global form
(WTGPU_FILM_ZONAL_LDS=0), the LDS form wherever the table fits 64 KB (=1; where it does not fit there is no entry) and with the knob unset (the
default, which is 1 with the global form where the table does not fit).  The knob
is read at the upload, so every form has a scene of its own over the same films.  Calls are alternated after a warm-up; each is timed between
device events (memset + edge upload + kernels + result copy); the median of --reps (>= 15) is reported, and the ratios to the yardsticks.
--kernel-only: every zonal call once per form and nothing else — for a kernel trace in a run of its own.
Films are seeded random numbers, log-uniform over eight decades.  Prints one JSON line and writes it to --out (default: profiles/film_zonal_bench.json).  Needs a GPU.  Not part of
bench.py."""
import argparse
import os

from film_bench_util import FILMS, alternate, event_ms, finish, log_uniform_films, need_gpu

FORMS = {"global": "0", "lds": "1", "default": None}
LDS_MAX = 64 << 10


def lds_bytes(n_zones, planes, bins):
    """kernels_zonal.hip: zonal_lds_bytes"""
    return ((bins + 2) & ~1) * 4 + n_zones * planes * (9 * 8 + 7 * 4 + 2 * 4 + bins * 4)


def upload(name, kw, lds):
    from wave_tracer_amd import Scene
    old = os.environ.get("WTGPU_FILM_ZONAL_LDS")
    if lds is None:
        os.environ.pop("WTGPU_FILM_ZONAL_LDS", None)
    else:
        os.environ["WTGPU_FILM_ZONAL_LDS"] = lds
    try:
        return Scene(name, **kw).upload(0, 65536)     # a small batch: nothing is rendered here
    finally:
        if old is None:
            os.environ.pop("WTGPU_FILM_ZONAL_LDS", None)
        else:
            os.environ["WTGPU_FILM_ZONAL_LDS"] = old


def zone_plans(H, W, dev):
    import torch
    from wave_tracer_amd.render import cell_zones
    g = torch.Generator(device=dev).manual_seed(7)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    cells, n_cells = cell_zones(H, W, 8)
    return {"halves_2": ((xx >= W // 2).int().contiguous(), 2, 256),
            "blocks_48": (((yy * 6 // H) * 8 + xx * 8 // W).int().contiguous(), 48, 256),
            "cells_8x8": (torch.from_numpy(cells.view("int32")).to(dev), n_cells, 32),
            "random_64": (torch.randint(0, 64, (H, W), device=dev, generator=g, dtype=torch.int32), 64, 256),
            "random_128": (torch.randint(0, 128, (H, W), device=dev, generator=g, dtype=torch.int32), 128, 256),      # 41 KB of table at three planes
            "random_200": (torch.randint(0, 200, (H, W), device=dev, generator=g, dtype=torch.int32), 200, 256),      # 64,808 bytes: all a launch may ask for
            "random_4096": (torch.randint(0, 4096, (H, W), device=dev, generator=g, dtype=torch.int32), 4096, 256)}


def bench_film(label, reps, kernel_only):
    import torch
    name, kw = FILMS[label]
    dev = torch.device("cuda", 0)
    scenes = {form: upload(name, kw, lds) for form, lds in FORMS.items()}
    sc = scenes["default"]
    H, W, P, planes = sc.height, sc.width, sc.channels, sc.spectral_channels
    _, value, weight, light = log_uniform_films(sc, dev)
    films, spe, rng = (value, weight, light), 16, (-60.0, 20.0)
    plans = zone_plans(H, W, dev)
    calls, fits = {}, {}
    for plan, (zones, Z, bins) in plans.items():
        for b in (0, bins):
            fits[f"{plan}/bins_{b}"] = lds_bytes(Z, planes, b)
            for form, s in scenes.items():
                if form == "lds" and lds_bytes(Z, planes, b) > LDS_MAX:
                    continue
                calls[f"{plan}/bins_{b}/{form}"] = (lambda s=s, zones=zones, Z=Z, b=b: s.film_zonal_device(films, spe, zones, Z, scale="dB", range=rng, bins=b))
    # both forms are exact: the same records
    for key, fn in calls.items():
        ref = calls[key.rsplit("/", 1)[0] + "/global"]()
        got = fn()
        assert all((got[k] == ref[k]).all() for k in ("n", "n_above", "hist")) and (got["sum"].view("uint64") == ref["sum"].view("uint64")).all(), key
    if kernel_only:
        torch.cuda.synchronize(dev)
        return {"film": [W, H, P], "calls": sorted(calls)}
    mask_a = (plans["halves_2"][0] == 0).float().contiguous()
    mask_b = (plans["halves_2"][0] == 1).float().contiguous()
    timed = {k: (lambda fn=fn: event_ms(fn)[0]) for k, fn in calls.items()}
    timed["stats_256"] = lambda: event_ms(lambda: sc.film_stats_device(*films, spe, range=rng, bins=256))[0]
    timed["stats_2_masked"] = lambda: event_ms(lambda: [sc.film_stats_device(*films, spe, range=rng, bins=256, mask=m) for m in (mask_a, mask_b)])[0]
    ms = alternate(timed, reps)
    films_bytes = int(8 * (2 * value.numel() + weight.numel()))
    out = {"film": [W, H, P], "bytes_f64_films": films_bytes, "lds_table_bytes": fits, "ms": ms,
           "ratio_to_stats_256": {k: v / ms["stats_256"] for k, v in ms.items() if "/" in k},
           "halves_2_over_stats_2_masked": {k: v / ms["stats_2_masked"] for k, v in ms.items() if k.startswith("halves_2/bins_256")}}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--films", default=",".join(FILMS))
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "film_zonal_bench.json"))
    args = ap.parse_args()
    need_gpu("bench_film_zonal")
    reps = max(15, args.reps)
    res = {"tool": "bench_film_zonal", "reps": reps, "kernel_only": args.kernel_only, "films": {f: bench_film(f, reps, args.kernel_only) for f in args.films.split(",")}}
    finish(res, args.out)


if __name__ == "__main__":
    main()
