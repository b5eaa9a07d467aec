#!/usr/bin/env python3
"""Times the question "how far apart are these two films" — count of differing elements, largest difference, relative L2 — the old way and the
new one, at the two full-size films: cornell (1440 x 1440, P = 3 planes) and the polarimetric room (1920 x 1088, P = 12).

  parent path   synchronise, copy the two sets of three f64 films to the host, wtgpu_develop each (one host thread), numpy on Stokes component 0:
                a != b, max |a - b| and its place, the sums of squares
  new path      Scene.film_compare_device: two kernels and a copy of the records (88 bytes per plane)

The two are alternated after a warm-up and the median of --reps (>= 15) is reported.  The call between two device events (which includes its
small copy) is reported apart, with and without the difference plane, with the bytes of the two film sets over that time: k_film_compare
reads every film byte once (of a polarimetric film the lines of all four Stokes components are fetched whole whichever is wanted), so that
quotient is to be held against the HBM read rate.  --kernel-only runs the device call alone a few times, for a kernel trace taken in a run of
its own.  Films are seeded random numbers, log-uniform over eight decades; B is A with noise of a few per cent.
Prints one JSON line; --out also writes it to a file.  Needs a GPU.  Not part of bench.py."""
import argparse
import sys
import time

from film_bench_util import FILMS, alternate, event_ms, finish, log_uniform_films, need_gpu


def make_films(label):
    import torch
    from wave_tracer_amd import Scene
    name, kw = FILMS[label]
    sc = Scene(name, **kw).upload(0, 65536)     # a small batch: nothing is rendered here
    dev = torch.device("cuda", 0)
    H, W, P = sc.height, sc.width, sc.channels
    g, value, weight, light = log_uniform_films(sc, dev)
    value_b = value * (1 + 0.03 * (torch.rand((H, W, P), dtype=torch.float64, device=dev, generator=g) - 0.5))
    value_b[::3] = value[::3]                   # a third of the rows agree exactly
    return sc, (value, weight, light), (value_b, weight.clone(), light.clone())


def bench_film(label, reps):
    import numpy as np
    import torch
    from wave_tracer_amd import develop
    sc, a, b = make_films(label)
    dev = torch.device("cuda", 0)
    H, W, stokes = sc.height, sc.width, sc.stokes
    spe = 16

    def parent():
        t0 = time.perf_counter()
        torch.cuda.synchronize(dev)
        ha, hb = (tuple(t.cpu().numpy() for t in f) for f in (a, b))
        t1 = time.perf_counter()
        xa, xb = (develop(sc, *f, spe).reshape(H * W, -1, stokes)[:, :, 0].astype(np.float64) for f in (ha, hb))
        t2 = time.perf_counter()
        d = xa - xb
        res = {"n_differ": (d != 0).sum(axis=0), "max_abs": np.abs(d).max(axis=0), "argmax": np.abs(d).argmax(axis=0),
               "rel_l2": np.sqrt((d * d).sum(axis=0) / (xb * xb).sum(axis=0))}
        t3 = time.perf_counter()
        return {"total_ms": (t3 - t0) * 1e3, "copy_ms": (t1 - t0) * 1e3, "develop_ms": (t2 - t1) * 1e3, "numpy_ms": (t3 - t2) * 1e3, "_res": res}

    def new():
        t0 = time.perf_counter()
        c = sc.film_compare_device(a, spe, b, spe)
        t1 = time.perf_counter()
        return {"total_ms": (t1 - t0) * 1e3, "_res": c}

    # the same answer: the counts and the maximum exactly, the quotient of sums to the rounding of numpy's own order of additions
    p, n = parent()["_res"], new()["_res"]
    agree = bool(np.array_equal(p["n_differ"], n["n_differ"].astype(np.int64)) and np.array_equal(p["max_abs"], n["max_abs"]) and
                 np.array_equal(p["argmax"], n["argmax"].astype(np.int64)) and np.allclose(p["rel_l2"], n["rel_l2"], rtol=1e-9, atol=0))
    strip = lambda fn: (lambda: {k: v for k, v in fn().items() if not k.startswith("_")})
    films_bytes = int(2 * 8 * (2 * a[0].numel() + a[1].numel()))
    planes = sc.spectral_channels
    out = {"film": [W, H, sc.channels], "bytes_two_f64_film_sets": films_bytes, "bytes_diff_plane": 4 * H * W * planes, "paths_agree": agree,
           "rel_l2": [float(x) for x in n["rel_l2"]], "n_differ": [int(x) for x in n["n_differ"]]}
    out.update(alternate({"parent": strip(parent), "new": strip(new)}, reps))
    out["new_back_to_back"] = alternate({"new": strip(new)}, reps)["new"]     # the new path alone, the GPU kept busy
    # one call = k_film_compare + k_film_finish + the copy of the records, between two device events
    lum = planes == 3
    passes = alternate({"records": lambda: {"ms": event_ms(lambda: sc.film_compare_device(a, spe, b, spe))[0]},
                         "records_luminance": lambda: {"ms": event_ms(lambda: sc.film_compare_device(a, spe, b, spe, luminance=lum))[0]},
                         "records_and_diff": lambda: {"ms": event_ms(lambda: sc.film_compare_device(a, spe, b, spe, diff=True))[0]},
                         "same_pointers": lambda: {"ms": event_ms(lambda: sc.film_compare_device(a, spe, a, spe))[0]}}, reps)
    out["device_events"] = {k: {"ms": v["ms"], "films_GBps": films_bytes / v["ms"] / 1e6} for k, v in passes.items()}
    return out


def kernel_only(label, calls):
    """The device call alone, for `rocprofv3 --kernel-trace --stats -- python tools/bench_film_compare.py --kernel-only`: k_film_compare's own
    time is in the trace's statistics."""
    import torch
    sc, a, b = make_films(label)
    for _ in range(calls):
        sc.film_compare_device(a, 16, b, 16)
    torch.cuda.synchronize()
    return {"film": [sc.width, sc.height, sc.channels], "bytes_two_f64_film_sets": int(2 * 8 * (2 * a[0].numel() + a[1].numel())), "calls": calls}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--films", default=",".join(FILMS))
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    need_gpu("bench_film_compare")
    if args.kernel_only:
        res = {"tool": "bench_film_compare", "kernel_only": {f: kernel_only(f, 20) for f in args.films.split(",")}}
    else:
        res = {"tool": "bench_film_compare", "reps": max(15, args.reps), "films": {f: bench_film(f, max(15, args.reps)) for f in args.films.split(",")}}
    finish(res, args.out)
    if not args.kernel_only and not all(f["paths_agree"] for f in res["films"].values()):
        sys.exit("the two paths disagree")


if __name__ == "__main__":
    main()
