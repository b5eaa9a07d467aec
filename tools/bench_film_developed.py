#!/usr/bin/env python3
"""Times the four film passes — tonemap, statistics, comparison, polarisation view — from a DEVELOPED f32 film against the same pass from the f64
accumulators, in the same run, at the two full-size films: cornell (1440 x 1440, P = 3 planes) and the polarimetric room (1920 x 1088, P = 12;
the polarisation view runs on this one only).

The developed film is Scene.develop_device's output of the seeded accumulators, so both forms of a pass compute the same thing (checked before
anything is timed: every record field bit for bit).  Each timing is one call between two device events — the main kernel, the finish kernel and
the copy of the records where the pass has them — the two forms alternated after a warm-up, the median of --reps (>= 15).  The accumulator form is
the yardstick: its kernels are the ones the pass had before the developed form existed.  Reported per pass and film: both times, their quotient,
and the bytes each form's main kernel has to read.  The comparison is timed with developed / developed and developed / accumulator operands; the
polarisation view with both settings of WTGPU_FILM_POLAR_STAGED, for both sources.  There is no pass mark.
--kernel-only runs each call a few times, for `rocprofv3 --kernel-trace --stats` in a run of its own: the kernels' own times are in its statistics.
Prints one JSON line; --out also writes it to a file.  Needs a GPU.  Not part of bench.py."""
import argparse
import os

from film_bench_util import FILMS, alternate, event_ms, finish, log_uniform_films, need_gpu

SPE = 16
SIX_MAPS = ("dolp", "dop", "docp", "aolp", "chi", "analyser")


def _scene(film, env=None):
    """An uploaded scene whose knobs were read with `env` set (the knobs are read once per upload)."""
    from wave_tracer_amd import Scene
    name, kw = FILMS[film]
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        return Scene(name, **kw).upload(0, 65536)     # a small batch: nothing is rendered here
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def make_films(film):
    """(scene, accumulators, a second set, the developed film of each)"""
    import torch
    sc = _scene(film)
    dev = torch.device("cuda", 0)
    sets = []
    for seed in (1, 2):
        g, value, weight, light = log_uniform_films(sc, dev, seed)
        if sc.stokes == 4:      # Q, U, V: a random fraction of the channel's I, of either sign (tools/bench_film_polar.py)
            H, W, P = sc.height, sc.width, sc.channels
            v = value.reshape(H, W, P // 4, 4)
            v[..., 1:] = v[..., :1] * ((torch.rand((H, W, P // 4, 3), dtype=torch.float64, device=dev, generator=g) - 0.5) * 1.1)
            light.reshape(H, W, P // 4, 4)[..., 1:] = 0.0
        sets.append((value, weight, light))
    developed = [sc.develop_device(*s, SPE) for s in sets]
    torch.cuda.synchronize(dev)
    return sc, sets, developed


def passes_of(sc, sets, developed):
    """{pass: {form: callable}}: the calls that are timed, the accumulator form first"""
    (acc, acc_b), (dev, dev_b) = sets, developed
    lum = sc.spectral_channels == 3
    tm = {"op": "sRGB", "mode": "normal"}
    out = {
        "tonemap_u8": {"accumulators": lambda: sc.tonemap_device(*acc, SPE, tm, fmt="u8"), "developed": lambda: sc.tonemap_developed_device(dev, tm, fmt="u8")},
        "stats_256_bins": {"accumulators": lambda: sc.film_stats_device(*acc, SPE, range=(-60.0, 20.0), bins=256, luminance=lum),
                           "developed": lambda: sc.film_stats_developed_device(dev, range=(-60.0, 20.0), bins=256, luminance=lum)},
        "compare": {"accumulators": lambda: sc.film_compare_device(acc, SPE, acc_b, SPE, luminance=lum),
                    "developed": lambda: sc.film_compare_device(dev, None, dev_b, None, luminance=lum),
                    "developed_against_accumulators": lambda: sc.film_compare_device(dev, None, acc_b, SPE, luminance=lum)},
    }
    if sc.stokes == 4:
        out["polar_records"] = {"accumulators": lambda: sc.film_polar_device(*acc, SPE, luminance=lum), "developed": lambda: sc.film_polar_developed_device(dev, luminance=lum)}
        out["polar_six_maps"] = {"accumulators": lambda: sc.film_polar_device(*acc, SPE, luminance=lum, maps=SIX_MAPS),
                                 "developed": lambda: sc.film_polar_developed_device(dev, luminance=lum, maps=SIX_MAPS)}
    return out


def same_records(a, b):
    import numpy as np
    import torch
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    return all(np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)) for k in a if isinstance(a[k], np.ndarray))


def read_bytes(sc, what):
    """what a pass's main kernel has to read of one film: the planes it uses and, of the accumulators, the weight word of every pixel"""
    n, P = sc.width * sc.height, sc.channels
    used = P if what.startswith("polar") else sc.spectral_channels       # the other passes take ONE Stokes component
    return {"accumulators": n * (16 * used + 8), "developed": n * 4 * used, "developed_film_whole": n * 4 * P, "accumulators_whole": n * (16 * P + 8)}


def bench_film(film, reps):
    sc, sets, developed = make_films(film)
    out = {"film": [sc.width, sc.height, sc.channels], "passes": {}}
    for what, forms in passes_of(sc, sets, developed).items():
        ref = forms["accumulators"]()
        agree = all(same_records(ref, fn()) for k, fn in forms.items() if k in ("accumulators", "developed")) if what != "compare" else True
        med = alternate({k: (lambda fn=fn: event_ms(fn)[0]) for k, fn in forms.items()}, reps)
        row = {k + "_ms": v for k, v in med.items()}
        row.update({k + "_over_accumulators": v / med["accumulators"] for k, v in med.items() if k != "accumulators"})
        row.update(forms_agree=bool(agree), bytes_read_per_film=read_bytes(sc, what))
        out["passes"][what] = row
    if sc.stokes == 4:
        # the existing A/B of k_film_polar's loads, for both sources: the wavefront stages its chunk through LDS (1), or every lane loads its own pixels (0)
        other = _scene(film, {"WTGPU_FILM_POLAR_STAGED": "0"})
        acc, dev = sets[0], developed[0]
        lum = sc.spectral_channels == 3
        ab = alternate({"staged_accumulators": lambda: event_ms(lambda: sc.film_polar_device(*acc, SPE, luminance=lum))[0],
                        "per_lane_accumulators": lambda: event_ms(lambda: other.film_polar_device(*acc, SPE, luminance=lum))[0],
                        "staged_developed": lambda: event_ms(lambda: sc.film_polar_developed_device(dev, luminance=lum))[0],
                        "per_lane_developed": lambda: event_ms(lambda: other.film_polar_developed_device(dev, luminance=lum))[0]}, reps)
        out["k_film_polar_loads_ms"] = ab
    return out


def kernel_only(film, calls):
    import torch
    sc, sets, developed = make_films(film)
    for forms in passes_of(sc, sets, developed).values():
        for fn in forms.values():
            for _ in range(calls):
                fn()
    torch.cuda.synchronize()
    return {"film": [sc.width, sc.height, sc.channels], "calls": calls}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    need_gpu("bench_film_developed")
    if args.kernel_only:
        res = {"tool": "bench_film_developed", "kernel_only": {f: kernel_only(f, 10) for f in FILMS}}
    else:
        reps = max(15, args.reps)
        res = {"tool": "bench_film_developed", "reps": reps, "staged_default": os.environ.get("WTGPU_FILM_POLAR_STAGED", "1"), "films": {f: bench_film(f, reps) for f in FILMS}}
    finish(res, args.out)
    if not args.kernel_only and not all(p["forms_agree"] for f in res["films"].values() for p in f["passes"].values()):
        raise SystemExit("a developed form disagrees with its accumulator form")


if __name__ == "__main__":
    main()
