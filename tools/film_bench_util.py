"""What the film benchmarks (bench_develop.py, bench_film_stats.py, bench_film_compare.py, bench_film_polar.py, bench_film_denoise.py, bench_film_denoise_guided.py) share: the two full-size films, the timing of
a call between device events, the alternation of the paths, the seeded log-uniform films and the one JSON line at the end."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FILMS = {"cornell_1440": ("cornell_box", dict(res=1440, mesh_detail=0, lut=(32, 32))),
         "bidir_room_1920_polarimetric": ("bidir_room", dict(res=1920, mesh_detail=0, lut=(32, 32), polarimetric=1))}


def event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def alternate(fns, reps, warmup=3):
    """fns: {label: callable -> ms or dict of ms}; every round calls each once, in turn.  Returns the medians."""
    rows = {k: [] for k in fns}
    for r in range(warmup + reps):
        for k, fn in fns.items():
            v = fn()
            if r >= warmup:
                rows[k].append(v)
    med = statistics.median
    return {k: ({f: med([x[f] for x in v]) for f in v[0]} if isinstance(v[0], dict) else med(v)) for k, v in rows.items()}


def log_uniform_films(sc, dev, seed=1):
    """(generator, value, weight, light): seeded f64 films on `dev`, the developed values log-uniform over eight decades."""
    import torch
    H, W, P = sc.height, sc.width, sc.channels
    g = torch.Generator(device=dev).manual_seed(seed)
    weight = torch.rand((H, W), dtype=torch.float64, device=dev, generator=g) * 40 + 1
    value = 10.0 ** (torch.rand((H, W, P), dtype=torch.float64, device=dev, generator=g) * 8 - 6) * weight[..., None]
    light = torch.rand((H, W, P), dtype=torch.float64, device=dev, generator=g) * 1e-7
    return g, value, weight, light


def need_gpu(tool):
    import torch
    if not torch.cuda.is_available():
        sys.exit(f"{tool}.py needs a GPU: a time taken anywhere else says nothing")


def finish(res, out):
    """Prints the result as one JSON line; `out`: also a file to write it to."""
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
