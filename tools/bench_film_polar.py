#!/usr/bin/env python3
"""Times the question "where and how strongly is this film polarised" — the degree-of-polarisation and angle maps of every channel and the
Stokes sums — the old way and the new one, at the full-size polarimetric film: the room (1920 x 1088, P = 12 planes).

  parent path   synchronise, copy the three f64 films to the host, wtgpu_develop (one host thread), numpy on the four Stokes components:
                dop, aolp, the sums over the lit pixels
  new path      Scene.film_polar_device: two kernels and a copy of the records (96 bytes per plane); the maps stay on the device

The two are alternated after a warm-up and the median of --reps (>= 15) is reported.  The call between two device events (which includes its
small copy) is reported apart — records alone, with the luminance's plane, with two maps, with all six, with the 8-bit picture — with the bytes of
the film set over that time, and beside it k_develop on the same film (Scene.develop_device), the yardstick of a kernel that reads every film
byte once: the quotient of the two times is reported, not judged.  --kernel-only runs the device call alone a few times, for a kernel trace taken
in a run of its own.  Films are seeded random numbers: intensities log-uniform over eight decades, Q / U / V of both signs within them.
Prints one JSON line; --out also writes it to a file.  Needs a GPU.  Not part of bench.py."""
import argparse
import os
import sys
import time

from film_bench_util import FILMS, alternate, event_ms, finish, log_uniform_films, need_gpu

FILM = "bidir_room_1920_polarimetric"
DEFAULT_STAGED = "1"      # the knob table's default for WTGPU_FILM_POLAR_STAGED


def _scene(env=None):
    """An uploaded scene whose knobs were read with `env` set (the knobs are read once per upload)."""
    from wave_tracer_amd import Scene
    name, kw = FILMS[FILM]
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        return Scene(name, **kw).upload(0, 65536)     # a small batch: nothing is rendered here
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def make_films():
    import torch
    sc = _scene()
    dev = torch.device("cuda", 0)
    H, W, P = sc.height, sc.width, sc.channels
    g, value, weight, light = log_uniform_films(sc, dev)
    # Q, U, V: a random fraction of the channel's I, of either sign, so that pol <= I in nearly every pixel
    v = value.reshape(H, W, P // 4, 4)
    frac = (torch.rand((H, W, P // 4, 3), dtype=torch.float64, device=dev, generator=g) - 0.5) * 1.1
    v[..., 1:] = v[..., :1] * frac
    light.reshape(H, W, P // 4, 4)[..., 1:] = 0.0
    return sc, (value, weight, light)


def bench_film(reps):
    import numpy as np
    import torch
    from wave_tracer_amd import develop
    sc, films = make_films()
    dev = torch.device("cuda", 0)
    H, W = sc.height, sc.width
    spe = 16

    def parent():
        t0 = time.perf_counter()
        torch.cuda.synchronize(dev)
        h = tuple(t.cpu().numpy() for t in films)
        t1 = time.perf_counter()
        s = develop(sc, *h, spe).reshape(H * W, -1, 4).astype(np.float64)
        t2 = time.perf_counter()
        i, q, u, v = (s[..., k] for k in range(4))
        lit = np.isfinite(s).all(axis=-1) & (i > 0)
        lin, pol = np.sqrt(q * q + u * u), np.sqrt((q * q + u * u) + v * v)
        with np.errstate(all="ignore"):
            dop, aolp = np.where(lit, pol / i, 0.0).astype(np.float32), np.where(lit, 0.5 * np.arctan2(u, q), 0.0).astype(np.float32)
        res = {"n_lit": lit.sum(axis=0), "max_dop": np.where(lit, pol / np.where(lit, i, 1.0), 0.0).max(axis=0), "sum_i": np.where(lit, i, 0.0).sum(axis=0),
               "sum_pol": np.where(lit, pol, 0.0).sum(axis=0), "dop": dop, "aolp": aolp}
        t3 = time.perf_counter()
        return {"total_ms": (t3 - t0) * 1e3, "copy_ms": (t1 - t0) * 1e3, "develop_ms": (t2 - t1) * 1e3, "numpy_ms": (t3 - t2) * 1e3, "_res": res}

    def new():
        t0 = time.perf_counter()
        c = sc.film_polar_device(*films, spe, maps=("dop", "aolp"))
        t1 = time.perf_counter()
        return {"total_ms": (t1 - t0) * 1e3, "_res": c}

    # the same answer: the counts, the maximum and the dop map exactly, the sums to the rounding of numpy's own order of additions, the angle
    # to the f32 ulp the library's arc tangent and libm's may differ by
    p, n = parent()["_res"], new()["_res"]
    n_lit = (n["n"] - n["n_nonfinite"] - n["n_dark"]).astype(np.int64)
    agree = bool(np.array_equal(p["n_lit"], n_lit) and np.array_equal(p["max_dop"], n["max_dop"]) and np.allclose(p["sum_i"], n["sum_i"], rtol=1e-9, atol=0) and
                 np.allclose(p["sum_pol"], n["sum_pol"], rtol=1e-9, atol=0) and np.array_equal(p["dop"], n["maps"]["dop"].cpu().numpy().reshape(p["dop"].shape)) and
                 np.abs(p["aolp"] - n["maps"]["aolp"].cpu().numpy().reshape(p["aolp"].shape)).max() <= 1.3e-7)
    strip = lambda fn: (lambda: {k: v for k, v in fn().items() if not k.startswith("_")})
    films_bytes = int(8 * (2 * films[0].numel() + films[1].numel()))
    planes = sc.spectral_channels
    out = {"film": [W, H, sc.channels], "bytes_f64_film_set": films_bytes, "bytes_per_map": 4 * H * W * planes, "paths_agree": agree,
           "mean_dop": [float(x) for x in n["mean_dop"]], "n_over": [int(x) for x in n["n_over"]]}
    out.update(alternate({"parent": strip(parent), "new": strip(new)}, reps))
    out["new_back_to_back"] = alternate({"new": strip(new)}, reps)["new"]     # the new path alone, the GPU kept busy
    # one call = k_film_polar + k_film_finish + the copy of the records, between two device events; k_develop beside it
    lum = planes == 3
    polar = lambda **kw: (lambda: {"ms": event_ms(lambda: sc.film_polar_device(*films, spe, **kw))[0]})
    passes = alternate({"records": polar(), "records_luminance": polar(luminance=lum), "records_and_two_maps": polar(maps=("dop", "aolp")),
                         "records_and_six_maps": polar(maps=("dolp", "dop", "docp", "aolp", "chi", "analyser")), "records_and_picture_u8": polar(picture=True, fmt="u8"),
                         "k_develop": lambda: {"ms": event_ms(lambda: sc.develop_device(*films, spe))[0]}}, reps)
    out["device_events"] = {k: {"ms": v["ms"], "films_GBps": films_bytes / v["ms"] / 1e6} for k, v in passes.items()}
    out["records_over_k_develop"] = passes["records"]["ms"] / passes["k_develop"]["ms"]
    # A/B: who loads the planes — every lane its own pixels' (96 bytes apart), or the wavefront its chunk's contiguously, through LDS
    other = _scene({"WTGPU_FILM_POLAR_STAGED": "0" if os.environ.get("WTGPU_FILM_POLAR_STAGED", DEFAULT_STAGED) == "1" else "1"})
    x, y = sc.film_polar_device(*films, spe, luminance=lum, maps=("dop", "aolp")), other.film_polar_device(*films, spe, luminance=lum, maps=("dop", "aolp"))
    assert all(np.array_equal(x[k], y[k]) for k in ("n", "n_over", "argmax", "max_dop", "sum_i", "sum_pol")) and all(torch.equal(x["maps"][k].view(torch.int32), y["maps"][k].view(torch.int32)) for k in x["maps"]), "the two forms differ"
    del x, y
    ab = alternate({"default": polar(), "other": lambda: {"ms": event_ms(lambda: other.film_polar_device(*films, spe))[0]},
                    "default_luminance_six_maps": polar(luminance=lum, maps=("dolp", "dop", "docp", "aolp", "chi", "analyser")),
                    "other_luminance_six_maps": lambda: {"ms": event_ms(lambda: other.film_polar_device(*films, spe, luminance=lum, maps=("dolp", "dop", "docp", "aolp", "chi", "analyser")))[0]}}, reps)
    staged_is_default = os.environ.get("WTGPU_FILM_POLAR_STAGED", DEFAULT_STAGED) == "1"
    name = {True: "staged", False: "per_lane"}
    out["k_film_polar_loads_ms"] = {name[staged_is_default]: ab["default"]["ms"], name[not staged_is_default]: ab["other"]["ms"],
                                    name[staged_is_default] + "_luminance_six_maps": ab["default_luminance_six_maps"]["ms"],
                                    name[not staged_is_default] + "_luminance_six_maps": ab["other_luminance_six_maps"]["ms"]}
    return out


def kernel_only(calls):
    """The device call alone, for `rocprofv3 --kernel-trace --stats -- python tools/bench_film_polar.py --kernel-only`: k_film_polar's own time is
    in the trace's statistics, k_develop's beside it."""
    import torch
    sc, films = make_films()
    for _ in range(calls):
        sc.film_polar_device(*films, 16)
        sc.develop_device(*films, 16)
    torch.cuda.synchronize()
    return {"film": [sc.width, sc.height, sc.channels], "bytes_f64_film_set": int(8 * (2 * films[0].numel() + films[1].numel())), "calls": calls}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    need_gpu("bench_film_polar")
    if args.kernel_only:
        res = {"tool": "bench_film_polar", "kernel_only": {FILM: kernel_only(20)}}
    else:
        res = {"tool": "bench_film_polar", "reps": max(15, args.reps), "films": {FILM: bench_film(max(15, args.reps))}}
    finish(res, args.out)
    if not args.kernel_only and not all(f["paths_agree"] for f in res["films"].values()):
        sys.exit("the two paths disagree")


if __name__ == "__main__":
    main()
