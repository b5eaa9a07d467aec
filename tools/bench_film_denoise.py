#!/usr/bin/env python3
"""Times the denoising of a film from its two half-films (the dual-buffer non-local-means filter; window 7, patch 2 unless told otherwise) the old
way and the new one, at the two full-size films: cornell (1440 x 1440, P = 3 planes) and the polarimetric room (1920 x 1088, P = 12).

  parent path   synchronise, copy the 2 x 3 f64 films to the host, wtgpu_develop (one host thread), a numpy restatement of the filter (f32,
                vectorised per window offset).  The restatement is run ONCE and on one tenth of the rows only ("numpy_rows"; it takes seconds per
                hundred rows): "numpy_ms_full_film_estimate" is that time x 10, an extrapolation, not a measurement.  The copy and the develop are
                measured on the whole film, alternated with the device call.
  new path      Scene.film_denoise_device: k_denoise_prepare, k_denoise_variance, k_denoise_filter; nothing crosses to the host

The device call between two device events is the median of --reps (>= 15), for the library's own choice and for both forms of k_denoise_filter forced
(WTGPU_FILM_DENOISE_FUSED: both directions in one launch, or one launch each), alternated, with and without the residual, and beside it k_develop on one of the two film sets
(Scene.develop_device), the yardstick of a kernel that reads every film byte once: the quotient is reported, not judged.  The two paths are
compared on the rows the restatement covers (largest difference relative to the film's largest value).  --kernel-only runs the device call alone a
few times, for a kernel trace taken in a run of its own.  Films: a smooth pattern with edges per plane and independent Gaussian noise (sigma 0.1) in
each half — a filter's time depends on how many weights are positive, so log-uniform noise would flatter it.
Prints one JSON line; --out also writes it to a file.  Needs a GPU.  Not part of bench.py."""
import argparse
import os
import sys
import time

from film_bench_util import FILMS, alternate, event_ms, finish, need_gpu

KNOB = "WTGPU_FILM_DENOISE_FUSED"      # 1 both directions in one launch, 0 one launch each; unset: the library chooses by the film's planes
SPE = 16


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


def make_halves(sc, sigma=0.1):
    import torch
    dev = torch.device("cuda", 0)
    H, W, P, stokes = sc.height, sc.width, sc.channels, sc.stokes
    g = torch.Generator(device=dev).manual_seed(1)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev), indexing="ij")
    truth = torch.empty((H, W, P), dtype=torch.float64, device=dev)
    for i in range(P):
        base = 0.5 + 0.3 * torch.sin(0.011 * xx + 0.007 * (i + 1) * yy) + 0.4 * (((xx // 160) + (yy // 120)) % 2)
        truth[..., i] = base if i % stokes == 0 else 0.2 * (base - 0.7)
    halves = []
    for _ in range(2):
        weight = torch.rand((H, W), dtype=torch.float64, device=dev, generator=g) * 40 + 1
        value = (truth + sigma * torch.randn((H, W, P), dtype=torch.float64, device=dev, generator=g)) * weight[..., None]
        halves.append((value, weight, torch.zeros((H, W, P), dtype=torch.float64, device=dev)))
    return halves


def restate_f32(a, b, stokes, r, f, k=0.45, alpha=1.0, eps=1e-10):
    """The filter in numpy f32 on developed films a, b [H, W, P] (all pixels finite, no mask): (fa + fb) / 2"""
    import numpy as np
    H, W, P = a.shape
    F = np.float32
    ya, yb = a[..., ::stokes], b[..., ::stokes]
    C_ = ya.shape[-1]
    ep = np.pad((ya - yb) ** 2 * F(0.5), ((1, 1), (1, 1), (0, 0)), mode="edge")
    v = sum(ep[j:j + H, i:i + W] for j in range(3) for i in range(3)) * F(1.0 / 9.0)
    uy, ux = np.clip(np.arange(-f, H + f), 0, H - 1), np.clip(np.arange(-f, W + f), 0, W - 1)
    out = []
    for x, y in ((a, yb), (b, ya)):
        yu, vu = y[uy][:, ux], v[uy][:, ux]
        sw, acc = np.zeros((H, W), F), np.zeros((H, W, P), F)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                qy, qx = np.clip(np.arange(-f, H + f) + dy, 0, H - 1), np.clip(np.arange(-f, W + f) + dx, 0, W - 1)
                yq, vq = y[qy][:, qx], v[qy][:, qx]
                s = (((yu - yq) ** 2 - F(alpha) * (vu + np.minimum(vu, vq))) / (F(eps) + F(k * k) * (vu + vq))).sum(axis=-1)
                h = sum(s[:, i:i + W] for i in range(2 * f + 1))
                D = sum(h[j:j + H] for j in range(2 * f + 1)) * F(1.0 / (C_ * (2 * f + 1) ** 2))
                w = np.where(D <= 0, F(1), np.exp(-np.maximum(D, F(0))))
                ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
                yt, xt = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
                wq = w[ys, xs]
                sw[ys, xs] += wq
                acc[ys, xs] += wq[..., None] * (x[yt, xt] - x[ys, xs])
        out.append(x + acc / sw[..., None])
    return (out[0] + out[1]) * F(0.5)


def bench_film(film, reps, window, patch):
    import numpy as np
    import torch
    from wave_tracer_amd import develop
    sc = _scene(film)
    forms = {"fused": _scene(film, {KNOB: "1"}), "two_launches": _scene(film, {KNOB: "0"})}
    dev = torch.device("cuda", 0)
    H, W, P = sc.height, sc.width, sc.channels
    a, b = make_halves(sc)
    kw = dict(window=window, patch=patch)

    def parent_io():
        t0 = time.perf_counter()
        torch.cuda.synchronize(dev)
        h = [tuple(t.cpu().numpy() for t in half) for half in (a, b)]
        t1 = time.perf_counter()
        d = [develop(sc, *half, SPE).reshape(H, W, P) for half in h]
        t2 = time.perf_counter()
        return {"copy_ms": (t1 - t0) * 1e3, "develop_ms": (t2 - t1) * 1e3, "_developed": d}

    def new():
        t0 = time.perf_counter()
        out = sc.film_denoise_device(a, SPE, b, SPE, **kw)
        torch.cuda.synchronize(dev)
        return {"total_ms": (time.perf_counter() - t0) * 1e3, "_res": out}

    # the restatement once, on a band of rows in the middle of the film (its halo of window + patch + 1 rows included, then cut off)
    rows, halo = max(16, H // 10), window + patch + 1
    y0 = (H - rows) // 2
    da, db = (t[y0 - halo:y0 + rows + halo] for t in parent_io()["_developed"])
    t0 = time.perf_counter()
    want = restate_f32(da, db, sc.stokes, window, patch)[halo:-halo]
    numpy_ms = (time.perf_counter() - t0) * 1e3
    got = new()["_res"]["film"].cpu().numpy().reshape(H, W, P)[y0:y0 + rows]
    diff = float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())
    x, y = (s.film_denoise_device(a, SPE, b, SPE, residual=True, **kw) for s in forms.values())
    assert all(torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)) for k in ("film", "residual")), "the two forms differ"
    del x, y
    strip = lambda fn: (lambda: {k: v for k, v in fn().items() if not k.startswith("_")})
    films_bytes = int(2 * 8 * (2 * a[0].numel() + a[1].numel()))
    out = {"film": [W, H, P], "window": window, "patch": patch, "bytes_f64_two_film_sets": films_bytes, "numpy_rows": rows, "numpy_ms_on_those_rows": numpy_ms,
           "numpy_ms_full_film_estimate": numpy_ms * H / rows, "largest_difference_rel": diff, "paths_agree": diff < 1e-4}
    out.update(alternate({"parent_copy_and_develop": strip(parent_io), "new": strip(new)}, reps))
    call = lambda s, **more: (lambda: {"ms": event_ms(lambda: s.film_denoise_device(a, SPE, b, SPE, **kw, **more))[0]})
    fns = {"default": call(sc), "default_residual": call(sc, residual=True)}
    for name, s in forms.items():
        fns[name], fns[name + "_residual"] = call(s), call(s, residual=True)
    fns["k_develop_one_half"] = lambda: {"ms": event_ms(lambda: sc.develop_device(*a, SPE))[0]}
    passes = alternate(fns, reps)
    out["device_events_ms"] = {k: v["ms"] for k, v in passes.items()}
    out["default_over_k_develop_of_both_halves"] = passes["default"]["ms"] / (2.0 * passes["k_develop_one_half"]["ms"])
    return out


def kernel_only(film, calls, window, patch):
    """The device call alone, for `rocprofv3 --kernel-trace --stats -- python tools/bench_film_denoise.py --kernel-only`: the three kernels' own times
    are in the trace's statistics, k_develop's beside them."""
    import torch
    sc = _scene(film)
    a, b = make_halves(sc)
    for _ in range(calls):
        sc.film_denoise_device(a, SPE, b, SPE, window=window, patch=patch)
        sc.develop_device(*a, SPE)
    torch.cuda.synchronize()
    return {"film": [sc.width, sc.height, sc.channels], "calls": calls}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--window", type=int, default=7)
    ap.add_argument("--patch", type=int, default=2)
    ap.add_argument("--films", default=",".join(FILMS))
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    need_gpu("bench_film_denoise")
    films = [f for f in args.films.split(",") if f]
    if args.kernel_only:
        res = {"tool": "bench_film_denoise", "kernel_only": {f: kernel_only(f, 5, args.window, args.patch) for f in films}}
    else:
        res = {"tool": "bench_film_denoise", "reps": max(15, args.reps), "films": {f: bench_film(f, max(15, args.reps), args.window, args.patch) for f in films}}
    finish(res, args.out)
    if not args.kernel_only and not all(f["paths_agree"] for f in res["films"].values()):
        sys.exit("the two paths disagree")


if __name__ == "__main__":
    main()
