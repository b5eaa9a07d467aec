#!/usr/bin/env python3
"""Times the connected segments of a label plane (Scene.film_segments_device: a union-find, seven kernels, the counts and the records back on the
host) at the two full-size films — cornell (1440 x 1440) and the polarimetric room (1920 x 1088) — in both forms of its first two phases: "tiled"
(WTGPU_FILM_SEGMENTS_TILED=1: a block labels a 64 x 32 tile in LDS, the global merge unions across tile borders only), "global" (=0: row runs of 64
pixels, every other link in global memory) and "default" (the knob unset).  The knob is read at the upload, so every form has a scene of its own.
Two yardsticks that the same run takes:

  zonal_halves     one Scene.film_zonal_device call without bins over two zones of the same film: a kernel this feature leaves untouched, the
                   cost of one streaming pass with atomics
  host_path        what the call replaces: the class plane down to the host, scipy.ndimage.label per class (the library's host twin where scipy
                   is absent; "host_labeller" says which), the segment plane up again — wall-clock time, median of --host-reps

Class planes: two halves; 48 coherent blocks; site percolation at p = 0.3, 0.593 (critical) and 0.9; a one-pixel spiral with the one-pixel gap
beside it (the longest chains of parents); the bundled etoile rendered at res 64, thresholded at its median and scaled up.  Each at both
connectivities.  Before anything is timed every form's result on every plane is held to the host twin's: plane, counts and records equal, and
the form each call took is read through the test hook.  Calls are
alternated after a warm-up; each is timed between device events (memsets + kernels + the copies of the result); the median of --reps (>= 15) is
reported, and the ratios to the yardsticks.  --kernel-only: every call once and nothing else — for a kernel trace in a run of its own.
Prints one JSON line and writes it to --out (default: profiles/film_segments_bench.json).  Needs a GPU.  Not part of bench.py."""
import argparse
import os
import statistics
import time

from film_bench_util import FILMS, alternate, event_ms, finish, log_uniform_films, need_gpu

NONE = 0xFFFFFFFF
FORMS = {"global": "0", "tiled": "1", "default": None}
KNOB = "WTGPU_FILM_SEGMENTS_TILED"


def upload(name, kw, tiled):
    from wave_tracer_amd import Scene
    old = os.environ.get(KNOB)
    if tiled is None:
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = tiled
    try:
        return Scene(name, **kw).upload(0, 65536)     # a small batch: nothing is rendered here
    finally:
        if old is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = old


def spiral(H, W):
    """class 1 along a one-pixel path that winds inwards from the corner, class 0 in the gap beside it"""
    import numpy as np
    g = [bytearray(W) for _ in range(H)]
    y = x = 0
    dy, dx = 0, 1
    g[0][0] = 1
    free = lambda v, u: not (0 <= v < H and 0 <= u < W) or g[v][u] == 0
    while True:
        for _ in range(2):
            v, u = y + dy, x + dx
            if 0 <= v < H and 0 <= u < W and g[v][u] == 0 and free(v + dy, u + dx):
                y, x = v, u
                g[y][x] = 1
                break
            dy, dx = dx, -dy
        else:
            break
    return np.frombuffer(b"".join(g), dtype=np.uint8).reshape(H, W).astype(np.uint32)


def etoile_holes(H, W):
    """the bundled etoile at res 64, 8 samples per element: 1 where the developed film lies below the median of its lit pixels, no class elsewhere; scaled up by
    repeating pixels"""
    import numpy as np
    from wave_tracer_amd import Scene, develop, render
    sc = Scene("etoile", res=64, mesh_detail=0)
    x = develop(sc, *render(sc, 8, seed=3, device=0), 8).reshape(sc.height, sc.width, -1)[..., 0]
    lit = x[x > 0]      # (most of the plane lies behind buildings and is exactly zero)
    assert lit.size, "the etoile film is dark"
    holes = np.where(x < np.median(lit), 1, NONE).astype(np.uint32)
    return holes[np.arange(H) * sc.height // H][:, np.arange(W) * sc.width // W]


def class_planes(H, W):
    import numpy as np
    yy, xx = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(7)
    planes = {"halves_2": (xx >= W // 2), "blocks_48": (yy * 6 // H) * 8 + xx * 8 // W}
    for p in (0.3, 0.593, 0.9):
        planes[f"percolation_{p}"] = np.where(rng.random((H, W)) < p, 1, NONE)
    planes["spiral"] = spiral(H, W)
    planes["etoile_holes"] = etoile_holes(H, W)
    return {k: np.ascontiguousarray(v.astype(np.uint32)) for k, v in planes.items()}


def host_labeller():
    """(name, fn(scene, classes uint32, diagonal) -> K): scipy.ndimage.label per class, or the host twin"""
    try:
        from scipy import ndimage
    except ImportError:
        return "host_twin", lambda sc, classes, diagonal: sc.film_segments_host(classes, diagonal=diagonal, max_records=0)["n_segments"]
    import numpy as np

    def label(sc, classes, diagonal):
        total = 0
        out = np.full(classes.shape, NONE, np.uint32)
        for c in np.unique(classes[classes != NONE]):
            lab, n = ndimage.label(classes == c, structure=np.ones((3, 3)) if diagonal else None)
            out[lab > 0] = (lab[lab > 0] + total - 1).astype(np.uint32)
            total += n
        label.plane = out
        return total
    return "scipy.ndimage.label", label


def bench_film(label, reps, host_reps, kernel_only):
    import numpy as np
    import torch
    from wave_tracer_amd import Scene
    from wave_tracer_amd.api import film_segments_form
    name, kw = FILMS[label]
    dev = torch.device("cuda", 0)
    scenes = {form: upload(name, kw, tiled) for form, tiled in FORMS.items()}
    sc = scenes["default"]
    H, W = sc.height, sc.width
    planes = class_planes(H, W)
    d_planes = {k: torch.from_numpy(v.view(np.int32)).to(dev) for k, v in planes.items()}
    calls, counts = {}, {}
    for plan, d in d_planes.items():
        for diagonal in (False, True):
            base = f"{plan}/{'8' if diagonal else '4'}"
            want = sc.film_segments_host(planes[plan], diagonal=diagonal)
            counts[base] = {"n_segments": want["n_segments"], "n_members": want["n_members"], "largest_recorded": int(want["area"].max()) if len(want["area"]) else 0}
            for form, s in scenes.items():
                key = f"{base}/{form}"
                calls[key] = lambda s=s, d=d, diagonal=diagonal: s.film_segments_device(d, diagonal=diagonal)
                # every form's result is the host twin's before anything is timed, and the call took the form it was asked for
                got = calls[key]()
                assert film_segments_form(s) == ("tiled" if form == "tiled" else "global", 0), (key, film_segments_form(s))
                assert all(got[k] == want[k] for k in ("n_segments", "n_dropped", "n_members", "n_dropped_pixels")), key
                assert all(np.array_equal(got[k], want[k]) for k in ("klass", "area", "first", "bbox", "centroid")), key
                assert np.array_equal(got["segments"].cpu().numpy().view(np.uint32), want["segments"]), key
    if kernel_only:
        torch.cuda.synchronize(dev)
        return {"film": [W, H], "calls": sorted(calls)}
    _, value, weight, light = log_uniform_films(sc, dev)
    timed = {k: (lambda fn=fn: event_ms(fn)[0]) for k, fn in calls.items()}
    timed["zonal_halves"] = lambda: event_ms(lambda: sc.film_zonal_device((value, weight, light), 16, d_planes["halves_2"], 2))[0]
    ms = alternate(timed, reps)
    how, labeller = host_labeller()
    host = {}
    for plan, d in d_planes.items():
        for diagonal in (False, True):
            rows = []
            for _ in range(host_reps):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                classes = d.cpu().numpy().view(np.uint32)
                k = labeller(sc, classes, diagonal)
                up = torch.from_numpy(getattr(labeller, "plane", classes).view(np.int32)).to(dev)
                torch.cuda.synchronize(dev)
                rows.append((time.perf_counter() - t0) * 1e3)
                del up
            key = f"{plan}/{'8' if diagonal else '4'}"
            assert k == counts[key]["n_segments"], (key, k)
            host[key] = statistics.median(rows)
    forms = {base: {form: ms[f"{base}/{form}"] for form in FORMS} for base in host}
    return {"film": [W, H], "segments": counts, "zonal_halves_ms": ms["zonal_halves"], "ms": forms, "host_path_ms": host, "host_labeller": how, "host_reps": host_reps,
            "tiled_over_global": {k: v["tiled"] / v["global"] for k, v in forms.items()},
            "ratio_to_zonal_halves": {k: {f: t / ms["zonal_halves"] for f, t in v.items()} for k, v in forms.items()},
            "host_path_over_device": {k: {f: host[k] / t for f, t in v.items()} for k, v in forms.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--films", default=",".join(FILMS))
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "film_segments_bench.json"))
    args = ap.parse_args()
    need_gpu("bench_film_segments")
    reps = max(15, args.reps)
    res = {"tool": "bench_film_segments", "reps": reps, "kernel_only": args.kernel_only,
           "films": {f: bench_film(f, reps, max(1, args.host_reps), args.kernel_only) for f in args.films.split(",")}}
    finish(res, args.out)


if __name__ == "__main__":
    main()
