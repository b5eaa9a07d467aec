#!/usr/bin/env python3
"""Times the question "which dB range does this film span, and how are its values distributed over it" — the range=None, bins=256 query — the
old way and the new one, at the two full-size films: cornell (1440 x 1440, P = 3 planes) and the polarimetric room (1920 x 1088, P = 12).

  parent path   synchronise, copy the three f64 films to the host, wtgpu_develop (one host thread), numpy: the smallest positive and the
                largest element, numpy.histogram of 10 log10 x over 256 bins between them
  new path      Scene.film_stats_device with range=None: two wtgpu_film_stats_device calls (the range pass without bins, then the histogram),
                each two kernels and a copy of a few hundred bytes to 8 KB

The two are alternated after a warm-up and the median of --reps (>= 15) is reported.  The kernels' own time (device events round one call,
which includes its small copies) is reported apart, per pass, with the bytes of the films over that time: k_film_stats reads every film byte
once (of a polarimetric film the lines of all four Stokes components are fetched whole whichever is wanted), so that quotient is to be held
against the HBM read rate.  Films are seeded random numbers, log-uniform over eight decades.
Prints one JSON line; --out also writes it to a file.  Needs a GPU.  Not part of bench.py."""
import argparse
import time

from film_bench_util import FILMS, alternate, event_ms, finish, log_uniform_films, need_gpu


def bench_film(label, reps):
    import numpy as np
    import torch
    from wave_tracer_amd import Scene, develop
    name, kw = FILMS[label]
    sc = Scene(name, **kw).upload(0, 65536)     # a small batch: nothing is rendered here
    dev = torch.device("cuda", 0)
    H, W, P, stokes = sc.height, sc.width, sc.channels, sc.stokes
    _, value, weight, light = log_uniform_films(sc, dev)
    spe = 16

    def parent():
        t0 = time.perf_counter()
        torch.cuda.synchronize(dev)
        v, w, l = (t.cpu().numpy() for t in (value, weight, light))
        t1 = time.perf_counter()
        img = develop(sc, v, w, l, spe)
        t2 = time.perf_counter()
        x = img.reshape(H * W, -1, stokes)[:, :, 0]
        pos = x[x > 0]
        lo, hi = 10 * np.log10(float(pos.min())), 10 * np.log10(float(x.max()))
        with np.errstate(divide="ignore", invalid="ignore"):
            hist = [np.histogram(10 * np.log10(x[:, c][x[:, c] > 0]), bins=256, range=(lo, hi))[0] for c in range(x.shape[1])]
        t3 = time.perf_counter()
        return {"total_ms": (t3 - t0) * 1e3, "copy_ms": (t1 - t0) * 1e3, "develop_ms": (t2 - t1) * 1e3, "numpy_ms": (t3 - t2) * 1e3, "_hist": hist}

    def new():
        t0 = time.perf_counter()
        st = sc.film_stats_device(value, weight, light, spe)
        t1 = time.perf_counter()
        return {"total_ms": (t1 - t0) * 1e3, "_hist": st["hist"]}

    # the same question: the library's range is 1e-3 dB wider at either end (so that both extremes fall inside), which moves every edge by up to
    # that much — 0.3 % of a bin's width — and a few elements per thousand into the neighbouring bin; the totals are the same but for an extreme that numpy's f32 logarithm puts outside its own range
    a, b = np.array(parent()["_hist"]), new()["_hist"].astype(np.int64)
    assert abs(int(a.sum()) - int(b.sum())) <= 2 * len(a) and np.abs(a - b).sum() <= 0.02 * a.sum(), "the two paths disagree"
    strip = lambda fn: (lambda: {k: v for k, v in fn().items() if not k.startswith("_")})
    films_bytes = int(8 * (2 * value.numel() + weight.numel()))
    out = {"film": [W, H, P], "bytes_f64_films": films_bytes}
    out.update(alternate({"parent": strip(parent), "new": strip(new)}, reps))
    out["new_back_to_back"] = alternate({"new": strip(new)}, reps)["new"]     # the new path alone, the GPU kept busy
    # one call = memset + edge upload + k_film_stats + k_film_stats_finish + result copy, between two device events
    lo, hi = sc.film_stats_device(value, weight, light, spe)["range"]
    passes = alternate({"range_pass": lambda: {"ms": event_ms(lambda: sc.film_stats_device(value, weight, light, spe, range=(0.0, 0.0), bins=0))[0]},
                         "histogram_pass": lambda: {"ms": event_ms(lambda: sc.film_stats_device(value, weight, light, spe, range=(lo, hi), bins=256))[0]},
                         "histogram_pass_4096": lambda: {"ms": event_ms(lambda: sc.film_stats_device(value, weight, light, spe, range=(lo, hi), bins=4096))[0]}}, reps)
    out["device_events"] = {k: {"ms": v["ms"], "films_GBps": films_bytes / v["ms"] / 1e6} for k, v in passes.items()}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--films", default=",".join(FILMS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    need_gpu("bench_film_stats")
    res = {"tool": "bench_film_stats", "reps": max(15, args.reps), "films": {f: bench_film(f, max(15, args.reps)) for f in args.films.split(",")}}
    finish(res, args.out)


if __name__ == "__main__":
    main()
