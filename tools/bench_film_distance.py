#!/usr/bin/env python3
"""Times the distance transform of a label plane (Scene.film_distance_device with nearest=True: a memset, k_dist_columns, k_dist_rows and the info
back on the host) at the two full-size films — cornell (1440 x 1440) and the polarimetric room (1920 x 1088) — in both forms of the row pass:
"groups" (WTGPU_FILM_DISTANCE_GROUPS=1: the outward search ends at |dx| = 64 and goes on group by group, skipping the 64-column groups that cannot
reach or tie the best), "plain" (=0: the outward search alone) and "default" (the knob unset).  The knob is read at the upload, so every form has
a scene of its own.  Yardsticks that the same run takes:

  segments         one Scene.film_segments_device call on the same plane, and
  zonal_halves     one Scene.film_zonal_device call without bins over two zones: parent kernels that this feature leaves untouched
  host_path        what the call replaces, where scipy imports: the plane down to the host, scipy.ndimage.distance_transform_edt(return_indices=True),
                   the squared distances and the indices up again — wall-clock time, median of --host-reps

Site planes, seeded: the right half; every other of 48 blocks; the bundled etoile rendered at res 64, thresholded at its median and scaled up
(tools/bench_film_segments.py's); site percolation at p = 0.5, 0.01 and 1e-5; one single site — the worst case of an outward search, whose cost
grows with the distance to the nearest site.  Before anything is timed every form's result on every plane is held to the host twin's — dist2,
nearest and the info equal — and the form each call took is read through the test hook.  Calls are alternated after a warm-up; each is timed
between device events; the median of --reps (>= 15) is reported, and the ratios to the yardsticks.  --kernel-only: every call once and nothing
else — for a kernel trace in a run of its own.  Prints one JSON line and writes it to --out (default: profiles/film_distance_bench.json).  Needs
a GPU.  Not part of bench.py."""
import argparse
import os
import statistics
import time

from bench_film_segments import etoile_holes
from film_bench_util import FILMS, alternate, event_ms, finish, log_uniform_films, need_gpu

NONE = 0xFFFFFFFF
FORMS = {"plain": "0", "groups": "1", "default": None}
KNOB = "WTGPU_FILM_DISTANCE_GROUPS"


def upload(name, kw, groups):
    from wave_tracer_amd import Scene
    old = os.environ.get(KNOB)
    if groups is None:
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = groups
    try:
        return Scene(name, **kw).upload(0, 65536)     # a small batch: nothing is rendered here
    finally:
        if old is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = old


def site_planes(H, W):
    import numpy as np
    yy, xx = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(7)
    planes = {"halves_2": np.where(xx >= W // 2, 1, NONE), "blocks_48": np.where(((yy * 6 // H) + (xx * 8 // W)) % 2 == 0, (yy * 6 // H) * 8 + xx * 8 // W, NONE),
              "etoile_holes": etoile_holes(H, W)}
    for p in (0.5, 0.01, 1e-5):
        planes[f"percolation_{p}"] = np.where(rng.random((H, W)) < p, 1, NONE)
    single = np.full((H, W), NONE)
    single[H // 3, W // 5] = 1
    planes["single_site"] = single
    return {k: np.ascontiguousarray(v.astype(np.uint32)) for k, v in planes.items()}


def bench_film(label, reps, host_reps, kernel_only):
    import numpy as np
    import torch
    from wave_tracer_amd.api import film_distance_form
    name, kw = FILMS[label]
    dev = torch.device("cuda", 0)
    scenes = {form: upload(name, kw, groups) for form, groups in FORMS.items()}
    sc = scenes["default"]
    H, W = sc.height, sc.width
    planes = site_planes(H, W)
    d_planes = {k: torch.from_numpy(v.view(np.int32)).to(dev) for k, v in planes.items()}
    calls, info, default_form = {}, {}, None
    for plan, d in d_planes.items():
        want = sc.film_distance_host(planes[plan], nearest=True)
        info[plan] = {k: want[k] for k in ("n_sites", "max_dist2", "argmax")}
        for form, s in scenes.items():
            key = f"{plan}/{form}"
            calls[key] = lambda s=s, d=d: s.film_distance_device(d, nearest=True)
            # every form's result is the host twin's before anything is timed, and the call took the form it was asked for
            got = calls[key]()
            took = film_distance_form(s)
            if form == "default":
                default_form = took
            else:
                assert took == form, (key, took)
            assert all(got[k] == want[k] for k in ("n_sites", "max_dist2", "argmax")), key
            assert all(np.array_equal(got[k].cpu().numpy().view(np.uint32), want[k]) for k in ("dist2", "nearest")), key
    if kernel_only:
        torch.cuda.synchronize(dev)
        return {"film": [W, H], "calls": sorted(calls)}
    _, value, weight, light = log_uniform_films(sc, dev)
    timed = {k: (lambda fn=fn: event_ms(fn)[0]) for k, fn in calls.items()}
    for plan, d in d_planes.items():
        timed[f"{plan}/segments"] = lambda d=d: event_ms(lambda: sc.film_segments_device(d, max_records=0))[0]
    d_halves = torch.from_numpy((np.mgrid[0:H, 0:W][1] >= W // 2).astype(np.int32)).to(dev)
    timed["zonal_halves"] = lambda: event_ms(lambda: sc.film_zonal_device((value, weight, light), 16, d_halves, 2))[0]
    ms = alternate(timed, reps)
    host = {}
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    if ndimage is not None:
        for plan, d in d_planes.items():
            rows = []
            for _ in range(host_reps):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                classes = d.cpu().numpy().view(np.uint32)
                edt, idx = ndimage.distance_transform_edt(classes == NONE, return_indices=True)
                d2 = np.rint(edt * edt).astype(np.uint32)
                near = (idx[0] * W + idx[1]).astype(np.uint32)
                up = (torch.from_numpy(d2.view(np.int32)).to(dev), torch.from_numpy(near.view(np.int32)).to(dev))
                torch.cuda.synchronize(dev)
                rows.append((time.perf_counter() - t0) * 1e3)
                del up
            assert int(d2.max()) == info[plan]["max_dist2"], (plan, int(d2.max()))
            host[plan] = statistics.median(rows)
    forms = {plan: {form: ms[f"{plan}/{form}"] for form in FORMS} for plan in d_planes}
    worst = max(forms, key=lambda p: forms[p]["default"])
    return {"film": [W, H], "planes": info, "default_form": default_form, "zonal_halves_ms": ms["zonal_halves"], "ms": forms,
            "segments_ms": {plan: ms[f"{plan}/segments"] for plan in d_planes}, "host_path_ms": host, "host_path": "scipy.ndimage.distance_transform_edt" if host else None,
            "host_reps": host_reps, "groups_over_plain": {k: v["groups"] / v["plain"] for k, v in forms.items()},
            "ratio_to_segments": {k: {f: t / ms[f"{k}/segments"] for f, t in v.items()} for k, v in forms.items()},
            "ratio_to_zonal_halves": {k: {f: t / ms["zonal_halves"] for f, t in v.items()} for k, v in forms.items()},
            "host_path_over_device": {k: {f: host[k] / t for f, t in v.items()} for k, v in forms.items()} if host else None,
            "worst_plane": {"plane": worst, "device_ms": forms[worst], "host_path_ms": host.get(worst)}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--films", default=",".join(FILMS))
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "film_distance_bench.json"))
    args = ap.parse_args()
    need_gpu("bench_film_distance")
    reps = max(15, args.reps)
    res = {"tool": "bench_film_distance", "reps": reps, "kernel_only": args.kernel_only,
           "films": {f: bench_film(f, reps, max(1, args.host_reps), args.kernel_only) for f in args.films.split(",")}}
    finish(res, args.out)


if __name__ == "__main__":
    main()
