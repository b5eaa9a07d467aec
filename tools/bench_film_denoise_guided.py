#!/usr/bin/env python3
"""Times the feature-guided denoiser (Scene.film_denoise_device(guide=, guide_scale=, ids=): the guided instantiations of k_denoise_filter) against
the unguided call in the same run, at the two full-size films of bench_film_denoise.py — cornell (1440 x 1440, P = 3 planes) and the polarimetric room
(1920 x 1088, P = 12) —, window 7, patch 2 unless told otherwise:

  unguided          Scene.film_denoise_device as before: the yardstick, which must also reproduce profiles/film_denoise_bench.json within run-to-run
                    noise (if it does not, the guided instantiations have disturbed the unguided ones)
  guided_global     G = 5 planes and ids, every lane reads g(q) from global memory where it reads x(q)        (WTGPU_FILM_DENOISE_GUIDE_LDS=0)
  guided_lds        the same, the candidate square's five planes staged in LDS beside the halo                (WTGPU_FILM_DENOISE_GUIDE_LDS=1)
  ids_only          SAME_ID alone: the id plane of the candidate square in LDS, no guide planes

Each is the median of --reps (>= 15) calls, alternated, every call with all its kernels between two device events.  The two guided forms must give
the same bits.  Films: bench_film_denoise.py's (a smooth pattern with a block pattern of edges, Gaussian noise of 0.1 in each half); guides: the
block indicator, three smooth planes and a stripe plane, noise-free, scales 2.78; ids: the block index.  How many weights the guides turn to 0
decides how many x(q) are read, so the guided times belong to these guides.
Prints one JSON line; --out also writes it to a file.  Needs a GPU.  Not part of bench.py."""
import argparse
import json
import os

from bench_film_denoise import SPE, _scene, make_halves
from film_bench_util import FILMS, alternate, event_ms, finish, need_gpu

KNOB = "WTGPU_FILM_DENOISE_GUIDE_LDS"      # 1 the guide planes of the candidate square in LDS where they fit, 0 from global memory
PARENT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "film_denoise_bench.json")


def make_guides(sc):
    """(guide [H, W, 5] f32, scales, ids [H, W] int32) on the device: what the films' pattern is made of, without the noise"""
    import torch
    dev = torch.device("cuda", 0)
    H, W = sc.height, sc.width
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=dev), torch.arange(W, dtype=torch.float32, device=dev), indexing="ij")
    bx, by = torch.div(xx, 160, rounding_mode="floor"), torch.div(yy, 120, rounding_mode="floor")
    planes = [(bx + by) % 2, 0.5 + 0.5 * torch.sin(0.011 * xx + 0.007 * yy), 0.5 + 0.5 * torch.sin(0.011 * xx + 0.021 * yy), torch.div(xx, 40, rounding_mode="floor") % 2,
              0.5 + 0.5 * torch.cos(0.005 * xx - 0.013 * yy)]
    return torch.stack(planes, dim=-1).contiguous(), [1.0 / 0.6 ** 2] * 5, (bx + 100 * by).to(torch.int32).contiguous()


def bench_film(film, reps, window, patch):
    import torch
    glob, lds = _scene(film, {KNOB: "0"}), _scene(film, {KNOB: "1"})
    a, b = make_halves(glob)
    guide, scales, ids = make_guides(glob)
    kw = dict(window=window, patch=patch)
    full = dict(guide=guide, guide_scale=scales, ids=ids)
    x, y = (s.film_denoise_device(a, SPE, b, SPE, residual=True, **kw, **full) for s in (glob, lds))
    plain = glob.film_denoise_device(a, SPE, b, SPE, residual=True, **kw)
    torch.cuda.synchronize()
    assert all(torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)) for k in ("film", "residual")), "the two guided forms differ"
    changed = float((x["film"].view(torch.int32) != plain["film"].view(torch.int32)).double().mean())
    del x, y, plain
    call = lambda s, **more: (lambda: event_ms(lambda: s.film_denoise_device(a, SPE, b, SPE, **kw, **more))[0])
    ms = alternate({"unguided": call(glob), "guided_global": call(glob, **full), "guided_lds": call(lds, **full), "ids_only": call(glob, ids=ids),
                    "unguided_residual": call(glob, residual=True), "guided_global_residual": call(glob, residual=True, **full),
                    "guided_lds_residual": call(lds, residual=True, **full)}, reps)
    out = {"film": [glob.width, glob.height, glob.channels], "window": window, "patch": patch, "guides": 5, "elements_changed_by_the_guides": changed,
           "device_events_ms": ms, "guided_global_over_unguided": ms["guided_global"] / ms["unguided"], "guided_lds_over_unguided": ms["guided_lds"] / ms["unguided"],
           "ids_only_over_unguided": ms["ids_only"] / ms["unguided"]}
    if os.path.exists(PARENT) and (window, patch) == (7, 2):
        parent = json.load(open(PARENT))["films"].get(film, {}).get("device_events_ms", {}).get("default")
        out["unguided_in_profiles_film_denoise_bench_json_ms"] = parent
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--window", type=int, default=7)
    ap.add_argument("--patch", type=int, default=2)
    ap.add_argument("--films", default=",".join(FILMS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    need_gpu("bench_film_denoise_guided")
    films = [f for f in args.films.split(",") if f]
    res = {"tool": "bench_film_denoise_guided", "reps": max(15, args.reps), "films": {f: bench_film(f, max(15, args.reps), args.window, args.patch) for f in films}}
    finish(res, args.out)


if __name__ == "__main__":
    main()
