"""Host-side render loop: the counterpart of scene_renderer_t::render / render_context_t::develop
(src/scene/render.cpp:381-579, 245-291).  Allocates the three linear film accumulators as torch tensors on the
GPU, calls the HIP path through the C-ABI and develops the film.  Multi-GPU: samples are sharded by sample index
(every rank renders all pixels for a disjoint sample range into its own film) and the films are summed with one
RCCL reduce — no collective on the data path."""
import ctypes as C

import numpy as np

from .api import FILM_ZONAL_NO_ZONE, Scene, load_library, _check


def alloc_films(scene, device):
    import torch
    H, W, Cn = scene.height, scene.width, scene.channels
    value = torch.zeros((H, W, Cn), dtype=torch.float64, device=device)
    weight = torch.zeros((H, W), dtype=torch.float64, device=device)
    light = torch.zeros((H, W, Cn), dtype=torch.float64, device=device)
    return value, weight, light


def develop(scene, value, weight, light, spe):
    """pixel = value/weight (0 where weight==0) + light/spe  — film_storage.hpp:256-287."""
    v = np.ascontiguousarray(value, dtype=np.float64)
    w = np.ascontiguousarray(weight, dtype=np.float64)
    l = np.ascontiguousarray(light, dtype=np.float64)
    out = np.zeros(v.shape, dtype=np.float32)
    _check(load_library().wtgpu_develop(scene.handle, v.ctypes.data, w.ctypes.data, l.ctypes.data, int(spe), out.ctypes.data))
    return out


def develop_device(scene, value, weight, light, spe, stream=None):
    """develop() where the films are: value / weight / light are the torch f64 films on the scene's device (alloc_films); returns the developed
    film as a numpy f32 array, bit for bit develop()'s.  Only the f32 result crosses to the host: half the bytes of one of the two f64 plane films."""
    import torch
    out = scene.develop_device(value, weight, light, spe, stream)
    torch.cuda.synchronize(out.device)
    return out.cpu().numpy()


def auto_db_range(scene, films, spe, *, percentiles=(1, 99), mask=None):
    """A dB range for the films as they are: the two percentiles of 10 log10 x over the positive elements (of the pixels where mask > 0), from a
    256-bin histogram between the smallest positive and the largest element — Scene.film_stats_device on torch films on the scene's device
    (nothing but counts crosses to the host), Scene.film_stats_host on numpy films.  An RGB film is judged by its luminance, a polarimetric
    one by its intensity (Stokes component 0).  Returns (db_min, db_max): tonemap_device's {"op": "dB", "db_range": ...}.
    films may also be ONE developed f32 film (a torch tensor on the scene's device: Scene.film_stats_developed_device, or a numpy array:
    Scene.film_stats_developed_host) — a denoised film, say; spe is then not read."""
    from . import imageio
    lum = scene.spectral_channels == 3
    if isinstance(films, (tuple, list)):
        value, weight, light = films
        stats_of = scene.film_stats_host if isinstance(value, np.ndarray) else scene.film_stats_device
        stats = stats_of(value, weight, light, spe, scale="dB", range=None, bins=256, luminance=lum, mask=mask)
    else:
        stats_of = scene.film_stats_developed_host if isinstance(films, np.ndarray) else scene.film_stats_developed_device
        stats = stats_of(films, scale="dB", range=None, bins=256, luminance=lum, mask=mask)
    lo, hi = imageio.percentiles(stats, percentiles)[-1 if lum else 0]
    return float(lo), float(hi)


def view(scene, film, tm=None, fmt="u8", mask=None, stokes_component=0):
    """A picture of a DEVELOPED film where it is: film is a torch f32 tensor [H, W, channels, stokes] on the scene's device (Scene.develop_device's
    result, a denoiser's "film" or "residual": Scene.tonemap_developed_device, the picture stays there) or a numpy float32 array
    (Scene.tonemap_developed_host).  tm: None = the scene's own tonemap_spec, else {op, mode, gamma, db_range, table}; a dB operator without a
    "db_range" takes auto_db_range's of this film (and this mask).  Returns tonemap_device's picture: H x W x 3 (x 4 with a mask) in `fmt`."""
    if tm is not None and tm.get("op") == "dB" and tm.get("db_range") is None:
        tm = dict(tm, db_range=auto_db_range(scene, film, None, mask=mask))
    tonemap = scene.tonemap_developed_host if isinstance(film, np.ndarray) else scene.tonemap_developed_device
    return tonemap(film, tm=tm, stokes_component=stokes_component, mask=mask, fmt=fmt)


_view = view    # (denoise has a keyword of the name)


def quality(scene, film, reference_films, reference_spe, **compare_kw):
    """How far is a DEVELOPED film — a denoised one — from a reference render?  film: a torch f32 tensor on the scene's device or a numpy float32
    array; reference_films = (value, weight, light), the accumulators of the reference (a long render) where the film is, developed with
    reference_spe samples per element.  compare_kw: Scene.film_compare_device's (stokes_component, abs, luminance, mask, eps, diff).  Returns that
    call's dict, film as A and the reference as B: the counts, max_abs / argmax, the sums, and rmse, mean_abs, rel_l2 = ||film - ref|| / ||ref||
    and rel_mse per plane.  Only the records cross to the host."""
    compare = scene.film_compare_host if isinstance(film, np.ndarray) else scene.film_compare_device
    return compare(film, None, reference_films, reference_spe, **compare_kw)


def noise_estimate(scene, films_a, films_b, spe, *, mask=None):
    """How noisy is the film that two half-films add up to?  films_a / films_b are (value, weight, light) of two renders of `spe` samples per element
    each over DISJOINT sample ranges (render_to_noise interleaves them), torch tensors on the scene's device (Scene.film_compare_device: only one
    record crosses to the host) or numpy arrays (Scene.film_compare_host).  Returns  ||a - b|| / ||a + b||  over the developed values of Stokes
    component 0 — the luminance of an RGB film, the one plane of a monochromatic one — of the pixels where mask > 0.  With independent halves of
    equal size, a - b has the variance of a + b, so the quotient estimates the relative RMS error of the merged film; it is an ESTIMATE: one
    draw of a random quantity, blind to any bias the two halves share.  Computed as  sqrt(sum_sq / (2 sum_a_sq + 2 sum_b_sq - sum_sq))  from three
    sums of squares (||a + b||^2 = 2 ||a||^2 + 2 ||b||^2 - ||a - b||^2), which spares the cancellation a sum of products a b would bring.  0 for
    two all-zero films."""
    compare = scene.film_compare_host if isinstance(films_a[0], np.ndarray) else scene.film_compare_device
    lum = scene.spectral_channels == 3
    c = compare(films_a, spe, films_b, spe, luminance=lum, mask=mask)
    k = -1 if lum else 0
    num, den = float(c["sum_sq"][k]), 2.0 * float(c["sum_a_sq"][k]) + 2.0 * float(c["sum_b_sq"][k]) - float(c["sum_sq"][k])
    return float(np.sqrt(num / den)) if den > 0 else 0.0


def polarisation(scene, films, spe, **kw):
    """Where and how strongly is the light of a polarimetric film polarised?  films = (value, weight, light), torch tensors on the scene's device
    (Scene.film_polar_device: the maps and the picture stay there, one record per plane crosses to the host) or numpy arrays
    (Scene.film_polar_host).  kw: luminance, maps, analyser, mask, picture, picture_plane, tm, fmt, sat_gain.  Returns that call's dict: counts,
    max_dop / argmax, the Stokes sums with dop_total, aolp_total, mean_dolp, mean_dop, "maps" by name, "picture"."""
    polar = scene.film_polar_host if isinstance(films[0], np.ndarray) else scene.film_polar_device
    return polar(*films, spe, **kw)


FIRST_HIT_GUIDE_KF = 0.6        # Rousselle, Manzi and Zwicker 2013's k_f; first_hit_guides' default scale is 1 / k_f^2 for every plane.  UNTUNED.


def first_hit_guides(scene, samples=0, seed=1, scales=None, same_shape=True, host=False):
    """The guides of a feature-guided denoise() from the scene's first-hit maps (Scene.first_hit on the scene's device; host=True: Scene.first_hit_host,
    numpy, no device needed): (guide, scales, ids) with guide [H, W, 5] f32 — the shading normal (3), the natural logarithm of the depth where the
    pixel is covered and 0 elsewhere (1), the coverage (1) —, scales the five plane scales and ids the shape map ([H, W]; None with
    same_shape=False).  Default scales: 1 / k_f^2 = 2.78 with k_f = 0.6 for every plane, the value Rousselle 2013 use on unit-range features; the
    log depth is not of unit range, and NOBODY HAS TUNED these numbers.  A sensor that is not perspective is refused by first_hit itself: pass
    guides of your own to denoise() for a virtual-plane sensor."""
    maps, ids = ("coverage", "depth", "normal_shading"), (("shape",) if same_shape else ())
    if scales is None:
        scales = [1.0 / FIRST_HIT_GUIDE_KF ** 2] * 5
    scales = [float(s) for s in np.broadcast_to(np.asarray(scales, dtype=np.float64), (5,))]
    if host:
        fh = scene.first_hit_host(samples, seed, maps, ids)
        cov = fh["coverage"] > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            logd = np.where(cov, np.log(np.where(cov, fh["depth"], np.float32(1))), np.float32(0)).astype(np.float32)
        guide = np.concatenate([fh["normal_shading"], logd[..., None], fh["coverage"][..., None]], axis=-1).astype(np.float32)
        return np.ascontiguousarray(guide), scales, (np.ascontiguousarray(fh["shape"]) if same_shape else None)
    import torch
    fh = scene.first_hit(samples, seed, maps, ids)
    cov = fh["coverage"] > 0
    logd = torch.where(cov, torch.log(torch.where(cov, fh["depth"], torch.ones_like(fh["depth"]))), torch.zeros_like(fh["depth"]))
    guide = torch.cat([fh["normal_shading"], logd[..., None], fh["coverage"][..., None]], dim=-1).contiguous()
    return guide, scales, (fh["shape"].contiguous() if same_shape else None)


def los_masks(scene, emitter=None, samples=0, seed=1, host=False):
    """The LOS / NLOS partition of a coverage map (Scene.line_of_sight on the scene's device; host=True: Scene.line_of_sight_host, numpy, no
    device needed): (los, nlos), two f32 arrays [H, W] of 1 and 0 that add up to 1 everywhere, ready for film_stats_device(mask=...) and the
    other film passes.  emitter: an index in the order of emitter_summary() — los is 1 where at least one of the element's samples sees that
    emitter (its VISIBLE > 0) —, or None: where it sees any emitter that is not an area emitter (N_VISIBLE > 0).  samples 0: the elements' centres."""
    query = scene.line_of_sight_host if host else scene.line_of_sight
    if emitter is None:
        seen = query(samples, seed, maps=(), ids=("n_visible",))["n_visible"] > 0
    else:
        seen = query(samples, seed, emitters=[int(emitter)], maps=("visible",), ids=())["visible"][..., 0] > 0
    if host:
        los = np.ascontiguousarray(seen, dtype=np.float32)
        return los, np.float32(1) - los
    los = seen.float().contiguous()
    return los, (1.0 - los).contiguous()


NO_ZONE = FILM_ZONAL_NO_ZONE    # the id of a pixel that belongs to no zone (the id maps' "no hit")


def zones_from_edges(plane, edges):
    """A zone plane from a plane of values: zone i where edges[i] <= x < edges[i + 1] (edges: strictly increasing, compared in the plane's own
    f32), 0xFFFFFFFF elsewhere — below the first edge, from the last edge on, NaN.  plane: a torch tensor [H, W] (the zones stay on its device, as
    int32 holding the u32 bits) or a numpy array (uint32).  Distance rings for the path-loss exponent come from line_of_sight's DISTANCE of one
    emitter or first_hit's DEPTH."""
    e = np.ascontiguousarray(edges, dtype=np.float32).reshape(-1)
    if e.size < 2 or not (np.diff(e.astype(np.float64)) > 0).all():
        raise ValueError("zones_from_edges: at least two strictly increasing edges (as float32) expected")
    if isinstance(plane, np.ndarray):
        x = plane.astype(np.float32, copy=False)
        inside = (x >= e[0]) & (x < e[-1])       # (False for a NaN)
        z = np.searchsorted(e, np.where(inside, x, e[0]), side="right") - 1
        return np.ascontiguousarray(np.where(inside, z, NO_ZONE).astype(np.uint32))
    import torch
    x = plane.float()
    te = torch.from_numpy(e).to(x.device)
    inside = (x >= te[0]) & (x < te[-1])
    z = torch.searchsorted(te, torch.where(inside, x, te[0]).contiguous(), right=True) - 1
    return torch.where(inside, z, torch.full_like(z, -1)).to(torch.int32).contiguous()


def cell_zones(height, width, cell):
    """Block cells as a zone plane (numpy uint32 [height, width]): cells of `cell` x `cell` pixels (the last of a row or column may be cut), numbered
    row-major — zone (y // cell) * ceil(width / cell) + x // cell — and their number."""
    cell = int(cell)
    if cell < 1 or height < 1 or width < 1:
        raise ValueError("cell_zones: positive sizes expected")
    per_row = -(-width // cell)
    yy, xx = np.mgrid[0:height, 0:width]
    return np.ascontiguousarray(((yy // cell) * per_row + xx // cell).astype(np.uint32)), per_row * -(-height // cell)


class ZonalStats(dict):
    """film_zonal_device's dict with percentiles(q) per zone."""

    def percentiles(self, q):
        """imageio.percentiles of every zone's histogram, in the histogram's own scale: [n_zones, planes] for one q, [n_zones, planes, len(q)] else."""
        from . import imageio
        if not self["bins"]:
            raise ValueError("zonal: percentiles need a histogram (bins > 0 and a range)")
        return np.stack([imageio.percentiles({"hist": self["hist"][z], "range": self["range"], "n_below": self["n_below"][z], "n_above": self["n_above"][z]}, q)
                         for z in range(self["n_zones"])])


def zonal(scene, films, spe, zones, n_zones=None, **kw):
    """Statistics per zone of a label plane in one pass over the films where they are: films = (value, weight, light) or one developed f32 film, torch
    tensors on the scene's device with zones there (Scene.film_zonal_device; a scene that is not uploaded yet is uploaded to the films' device) or
    numpy arrays (Scene.film_zonal_host).  kw: stokes_component, abs, luminance, mask, scale, range, bins, paint.  Returns that call's dict, which
    also answers percentiles(q) per zone from the histograms."""
    first = films[0] if isinstance(films, (tuple, list)) else films
    if isinstance(first, np.ndarray):
        return ZonalStats(scene.film_zonal_host(films, spe, zones, n_zones, **kw))
    if scene.device is None:
        scene.upload(first.device.index or 0)
    return ZonalStats(scene.film_zonal_device(films, spe, zones, n_zones, **kw))


def coverage_by_los(scene, films, spe, emitter=None, samples=0, seed=1, **kw):
    """Received power without and under line of sight in ONE pass: zonal() over two zones, 0 = no line of sight and 1 = line of sight, from
    Scene.line_of_sight's n_visible > 0 (emitter=None: any emitter that is not an area emitter) or one emitter's visible > 0, computed where the
    films are (numpy films: the host twins).  kw: zonal()'s."""
    first = films[0] if isinstance(films, (tuple, list)) else films
    host = isinstance(first, np.ndarray)
    if not host and scene.device is None:
        scene.upload(first.device.index or 0)
    los, _ = los_masks(scene, emitter, samples, seed, host=host)
    zones = np.ascontiguousarray(los > 0, dtype=np.uint32) if host else (los > 0).int().contiguous()
    return zonal(scene, films, spe, zones, 2, **kw)


def segments(scene, classes=None, **kw):
    """The connected segments of a label plane where it is: classes (or, with classes=None, kw["mask"]) a torch tensor on the scene's device
    (Scene.film_segments_device; a scene that is not uploaded yet is uploaded to that device) or a numpy array (Scene.film_segments_host).
    kw: mask, diagonal, min_area, max_records, and stream or threads.  Returns that call's dict."""
    first = classes if classes is not None else kw.get("mask")
    if first is None or isinstance(first, np.ndarray):
        if first is None and scene.device is not None:
            return scene.film_segments_device(classes, **kw)
        return scene.film_segments_host(classes, **kw)
    if scene.device is None:
        scene.upload(first.device.index or 0)
    return scene.film_segments_device(classes, **kw)


COVERAGE_HOLES_MAX_ZONES = 65536   # the zonal statistics' limit


def coverage_holes(scene, films, spe, threshold, *, scale="dB", below=True, stokes_component=0, channel=0, mask=None, min_area=1, diagonal=False, **zonal_kw):
    """The coverage holes of a film — the connected areas where one plane of the developed film lies below a threshold (below=False: at or above
    it) — and the film's statistics inside each, computed where the films are: films = (value, weight, light) or one developed f32 film, torch
    tensors on the scene's device or numpy arrays (the host twins).  The plane is spectral channel `channel` of Stokes component
    stokes_component; it is compared in its own f32 scale with the threshold as an f32 — for scale="dB" 10^(threshold / 10), converted once on the
    host (wtgpu_film_stats_edges, as film_stats does).  A NaN is in no hole.  A hole is a segment (segments(): mask, min_area, diagonal) of the
    class plane that holds 1 in the hole pixels and NO_ZONE elsewhere.  Returns segments()'s dict with "threshold" (the f32 compared against) and
    "zonal": zonal() over the holes (in the same scale; zonal_kw: abs, luminance, range, bins, paint), so that zonal["n"][i] is the area of hole i.  zonal()
    reports EVERY plane of the film's Stokes component, not only the thresholded one: the plane the holes were cut from is column `channel` of its
    arrays (zonal["max"][:, channel] lies below the threshold for below=True) — or None,
    with "zonal_skipped" saying why, where there is no hole or there are more than 65536 of them."""
    import ctypes as C
    from .api import FILM_STATS_SCALES, FilmStatsSpec
    if scale not in FILM_STATS_SCALES:
        raise ValueError(f"coverage_holes: scale 'dB' or 'linear' expected, got {scale!r}")
    if not 0 <= int(channel) < scene.spectral_channels or not 0 <= int(stokes_component) < scene.stokes:
        raise ValueError(f"coverage_holes: channel {channel} / stokes_component {stokes_component} out of range ({scene.spectral_channels} channels, {scene.stokes} Stokes components)")
    edge = np.zeros(1, dtype=np.float32)
    fs = FilmStatsSpec(0, FILM_STATS_SCALES.index(scale), 0, 0, float(threshold), 0.0)
    _check(load_library().wtgpu_film_stats_edges(C.byref(fs), edge.ctypes.data))
    first = films[0] if isinstance(films, (tuple, list)) else films
    host = isinstance(first, np.ndarray)
    shape = (scene.height, scene.width, scene.spectral_channels, scene.stokes)
    if host:
        developed = develop(scene, *films, spe) if isinstance(films, (tuple, list)) else films
        x = developed.reshape(shape)[:, :, int(channel), int(stokes_component)]
        inside = x < edge[0] if below else x >= edge[0]       # (False for a NaN either way)
        classes = np.ascontiguousarray(np.where(inside, 1, NO_ZONE).astype(np.uint32))
    else:
        import torch
        if scene.device is None:
            scene.upload(first.device.index or 0)
        developed = scene.develop_device(*films, spe) if isinstance(films, (tuple, list)) else films
        x = developed.reshape(shape)[:, :, int(channel), int(stokes_component)]
        thr = float(edge[0])                                    # (an f32's value: the comparison with the f32 plane is exact)
        inside = x < thr if below else x >= thr
        classes = torch.where(inside, 1, -1).to(torch.int32).contiguous()
    out = segments(scene, classes, mask=mask, min_area=min_area, diagonal=diagonal)
    out["threshold"] = edge[0]
    out["zonal"] = None
    if out["n_segments"] == 0:
        out["zonal_skipped"] = "no segments"
    elif out["n_segments"] > COVERAGE_HOLES_MAX_ZONES:
        out["zonal_skipped"] = f"{out['n_segments']} segments: more than the {COVERAGE_HOLES_MAX_ZONES} zones the zonal statistics hold (raise min_area)"
    else:
        out["zonal"] = zonal(scene, films, spe, out["segments"], out["n_segments"], stokes_component=stokes_component, mask=mask, scale=scale, **zonal_kw)
    return out


def distance(scene, classes=None, **kw):
    """The exact Euclidean distance transform of a label plane where it is: classes (or, with classes=None, kw["mask"]) a torch tensor on the
    scene's device (Scene.film_distance_device; a scene that is not uploaded yet is uploaded to that device) or a numpy array
    (Scene.film_distance_host).  kw: mask, invert, nearest, and stream or threads.  Returns that call's dict."""
    first = classes if classes is not None else kw.get("mask")
    if first is None or isinstance(first, np.ndarray):
        if first is None and scene.device is not None:
            return scene.film_distance_device(classes, **kw)
        return scene.film_distance_host(classes, **kw)
    if scene.device is None:
        scene.upload(first.device.index or 0)
    return scene.film_distance_device(classes, **kw)


def _radius2(what, radius):
    """the integer floor(radius²) that a squared pixel distance is compared with (below 2^31, above every distance of a sensor the pass takes)"""
    import math
    from fractions import Fraction
    if not (math.isfinite(radius) and radius >= 0):
        raise ValueError(f"{what}: a finite radius >= 0 expected, got {radius!r}")
    return min(math.floor(Fraction(radius) ** 2), 2 ** 31 - 1)


def _bool_plane(what, plane):
    """a bool plane as the f32 mask whose members (> 0) are its True pixels"""
    if isinstance(plane, np.ndarray):
        if plane.dtype != np.bool_:
            raise ValueError(f"{what}: a bool plane expected, got {plane.dtype}")
        return np.ascontiguousarray(plane, dtype=np.float32)
    import torch
    if not isinstance(plane, torch.Tensor) or plane.dtype != torch.bool:
        raise ValueError(f"{what}: a bool plane (torch or numpy) expected")
    return plane.float().contiguous()


def _dist2_u32(dist2):
    """dist2 as signed 64-bit numbers holding the u32 values (torch keeps the bits in int32)"""
    if isinstance(dist2, np.ndarray):
        return dist2.view(np.uint32).astype(np.int64)
    return dist2.long() & 0xFFFFFFFF


def dilate(scene, plane, radius):
    """Dilation of a bool plane (torch on the scene's device, or numpy) by a disc: True where a True pixel lies within `radius` pixels, centre to
    centre — dist2 <= floor(radius²), an integer comparison.  One distance() call.  The film's outside holds no site: nothing grows in from beyond
    the border."""
    r2 = _radius2("dilate", radius)
    return _dist2_u32(distance(scene, mask=_bool_plane("dilate", plane))["dist2"]) <= r2


def erode(scene, plane, radius):
    """Erosion of a bool plane by a disc: True where no False pixel lies within `radius` pixels — the inverted transform's dist2 >
    floor(radius²).  One distance() call.  The film's outside holds no site, so a region touching the border is not eroded from that side (scipy's
    binary_erosion with border_value=1)."""
    r2 = _radius2("erode", radius)
    return _dist2_u32(distance(scene, mask=_bool_plane("erode", plane), invert=True)["dist2"]) > r2


def opening(scene, plane, radius):
    """erode, then dilate, by the same disc (two distance() calls): drops what is thinner than the disc — one-pixel bridges, specks.  The film's
    outside holds no site, so a region touching the border is not eroded from that side."""
    return dilate(scene, erode(scene, plane, radius), radius)


def closing(scene, plane, radius):
    """dilate, then erode, by the same disc (two distance() calls): fills what is thinner than the disc — pin-holes, one-pixel gaps.  The film's
    outside holds no site, so a region touching the border is not eroded from that side."""
    return erode(scene, dilate(scene, plane, radius), radius)


def nearest_segment(scene, segments_plane):
    """The Voronoi partition of a segments plane (segments()'s "segments", or any zone plane): every pixel gets the number of the segment whose
    nearest pixel is nearest to it — segments.flatten()[nearest], of several equally far pixels the one with the smallest index — and NO_ZONE
    where the plane holds no segment at all.  A zone plane that zonal() takes as it is (torch int32 holding the u32 bits, or numpy uint32)."""
    near = distance(scene, segments_plane, nearest=True)["nearest"]
    if isinstance(near, np.ndarray):
        none = near == NO_ZONE
        out = segments_plane.reshape(-1).view(np.uint32)[np.where(none, 0, near)]
        return np.ascontiguousarray(np.where(none, NO_ZONE, out).astype(np.uint32))
    import torch
    none = near < 0
    out = segments_plane.reshape(-1)[torch.where(none, torch.zeros_like(near), near).long()]
    return torch.where(none, torch.full_like(out, -1), out).to(torch.int32).contiguous()


def zones_from_distance(dist2, edges_px):
    """Distance rings around the sites of a distance transform as a zone plane: zone i where edges_px[i]² <= d² < edges_px[i + 1]² (edges_px: at
    least two, not negative, strictly increasing, in pixels), compared in integers against ceil(edge²); NO_ZONE elsewhere and where d² is
    0xFFFFFFFF, no site.  dist2: distance()'s "dist2", a torch tensor (the zones stay on its device, as int32 holding the u32 bits) or a numpy
    array (uint32)."""
    import math
    from fractions import Fraction
    e = [float(v) for v in np.ravel(edges_px)]
    if len(e) < 2 or not all(math.isfinite(v) and v >= 0 for v in e) or not all(a < b for a, b in zip(e, e[1:])):
        raise ValueError("zones_from_distance: at least two finite, not negative, strictly increasing edges expected")
    t = np.array([min(math.ceil(Fraction(v) ** 2), 2 ** 32 - 1) for v in e], dtype=np.int64)   # (d² < 2^32 - 1 always holds for a site's d²)
    d = _dist2_u32(dist2)
    if isinstance(d, np.ndarray):
        inside = (d >= t[0]) & (d < t[-1])
        z = np.searchsorted(t, d, side="right") - 1
        return np.ascontiguousarray(np.where(inside, z, NO_ZONE).astype(np.uint32))
    import torch
    tt = torch.from_numpy(t).to(d.device)
    inside = (d >= tt[0]) & (d < tt[-1])
    z = torch.searchsorted(tt, d.contiguous(), right=True) - 1
    return torch.where(inside, z, torch.full_like(z, -1)).to(torch.int32).contiguous()


SHADOW_GUIDE_SCALE = 1.0 / FIRST_HIT_GUIDE_KF ** 2   # shadow_guides' default scale for every plane: first_hit_guides' 2.78.  UNTUNED.
SHADOW_GUIDE_T_MIN = 1e-4                            # shadow_guides' default t_min, in diagonals of the scene's bounding box


def shadow_guides(scene, samples=0, seed=1, scales=None, t_min=None, emitters=None, host=False):
    """Noise-free shadow planes of a perspective sensor as guides of a feature-guided denoise(): from every pixel's first-hit position
    (Scene.first_hit's position and normal_geo over `samples` primary rays, its coverage as the mask), is each lamp visible
    (Scene.line_of_sight(points=..., normals=..., t_min=...), front_only off: a first-hit normal is not turned towards the camera)?  Returns (guide,
    scales, None) as denoise(guides=...) takes it: guide [H, W, E] f32 on the scene's device (host=True: numpy from the host twins, no device
    needed), 1 where pixel and lamp see each other, 0 in the lamp's shadow and where the pixel sees nothing; E: the emitters that are not area
    emitters (or `emitters`), at most 8 for the denoiser.  t_min defaults to 1e-4 x the diagonal of the scene's bounding box.  The scales
    default to 2.78 for every plane as first_hit_guides' do and are UNTUNED: nobody has measured a denoise with these guides.  A sensor that is
    not perspective is refused by first_hit itself."""
    fh = (scene.first_hit_host if host else scene.first_hit)(samples, seed, maps=("coverage", "position", "normal_geo"), ids=())
    if t_min is None:
        st = scene.stats()
        t_min = SHADOW_GUIDE_T_MIN * float(np.linalg.norm(np.asarray(st["world_max"], dtype=np.float64) - np.asarray(st["world_min"], dtype=np.float64)))
    points, normals, mask = ((np.ascontiguousarray(fh[k]) if host else fh[k].contiguous()) for k in ("position", "normal_geo", "coverage"))
    guide = (scene.line_of_sight_host if host else scene.line_of_sight)(0, seed, emitters=emitters, maps=("visible",), ids=(), front_only=False, points=points,
                                                                        normals=normals, mask=mask, t_min=t_min)["visible"]
    guide = np.ascontiguousarray(guide) if host else guide.contiguous()
    if scales is None:
        scales = SHADOW_GUIDE_SCALE
    return guide, [float(s) for s in np.broadcast_to(np.asarray(scales, dtype=np.float64), (guide.shape[-1],))], None


MATERIAL_GUIDE_SCALE = 1.0 / FIRST_HIT_GUIDE_KF ** 2   # material_guides' default scale for every plane: first_hit_guides' 2.78.  UNTUNED.


def material_guides(scene, samples=0, seed=1, scales=None, host=False):
    """A noise-free reflectance plane per spectral channel as guides of a feature-guided denoise(): albedo + specular + emission of
    Scene.first_hit_material at Scene.channel_wavenumbers(), clamped to [0, 1] — what a checkerboard, a bitmap or a mask pattern on a flat wall
    changes while every geometric guide stays constant.  Returns (guide, scales, None) as denoise(guides=...) takes it: guide [H, W, C] f32 on the
    scene's device (host=True: numpy from the host twin, no device needed), C the spectral channels.  The scales default to 2.78 for every plane
    as first_hit_guides' do and are UNTUNED.  A sensor that is not perspective is refused by first_hit_material itself."""
    fm = (scene.first_hit_material_host if host else scene.first_hit_material)(samples, seed, None, ("albedo", "specular", "emission"), ())
    total = fm["albedo"] + fm["specular"] + fm["emission"]
    guide = np.ascontiguousarray(np.clip(total, np.float32(0), np.float32(1)), dtype=np.float32) if host else total.clamp(0.0, 1.0).contiguous()
    if scales is None:
        scales = MATERIAL_GUIDE_SCALE
    return guide, [float(s) for s in np.broadcast_to(np.asarray(scales, dtype=np.float64), (guide.shape[-1],))], None


def join_guides(*triples):
    """Joins (guide, scales, ids) triples — first_hit_guides, shadow_guides, material_guides, or a caller's — into one for denoise(guides=...): the
    planes and their scales concatenated in the order given, the ids of the first triple that has any.  All on the host (numpy) or all on one
    device (torch).  More than 8 planes are refused: the guided filter takes no more."""
    from .api import FILM_DENOISE_MAX_GUIDES
    if not triples:
        raise ValueError("join_guides: at least one (guide, scales, ids) triple expected")
    planes, scales, ids = [], [], None
    for guide, sc, i in triples:
        if guide is not None:
            guide = guide if guide.ndim == 3 else guide[..., None]
            if len(sc) != guide.shape[-1]:
                raise ValueError(f"join_guides: {guide.shape[-1]} planes with {len(sc)} scales")
            planes.append(guide)
            scales += [float(s) for s in sc]
        if ids is None and i is not None:
            ids = i
    if len(scales) > FILM_DENOISE_MAX_GUIDES:
        raise ValueError(f"join_guides: {len(scales)} planes, the guided filter takes at most {FILM_DENOISE_MAX_GUIDES}")
    if not planes:
        return None, [], ids
    if isinstance(planes[0], np.ndarray):
        return np.ascontiguousarray(np.concatenate(planes, axis=-1), dtype=np.float32), scales, ids
    import torch
    return torch.cat(planes, dim=-1).contiguous(), scales, ids


def denoise(scene, films_a, films_b, spe, guides=None, view=None, **kw):
    """Denoises the film that the half-films A and B add up to (render_to_noise(..., halves=True); `spe` samples per element each): films_a / films_b
    are (value, weight, light), torch tensors on the scene's device (Scene.film_denoise_device: everything stays there) or numpy arrays
    (Scene.film_denoise_host).  kw: window, patch, k, alpha, eps, mask, residual (default here: True).  Returns that call's dict — "film", "residual" —
    and "residual_rel" = ||residual|| / ||film|| over the guide planes (Stokes component 0 of each channel) of the pixels where both are finite: an
    ESTIMATE of the relative error that is left, from the difference of the two filtered halves (None with residual=False; 0 for an all-zero film).
    guides: None (the colour-only filter, as before), a (guide, scales, ids) triple as first_hit_guides returns it — arrays where the films are; ids or
    guide may be None — or True: first_hit_guides(scene) with its untuned defaults, on the host for numpy films.
    view: None (the dict is as above), True or a dict of view()'s keywords (tm, fmt, mask, stokes_component): adds "picture", view() of the
    denoised film where it is."""
    on_host = isinstance(films_a[0], np.ndarray)
    if guides is not None and guides is not False:
        guide, scales, ids = first_hit_guides(scene, host=on_host) if guides is True else guides
        kw = dict(kw, guide=guide, guide_scale=None if guide is None else scales, ids=ids)
    out = (scene.film_denoise_host if on_host else scene.film_denoise_device)(films_a, spe, films_b, spe, **dict({"residual": True}, **kw))
    out["residual_rel"] = None
    if out["residual"] is not None:
        film, res = (t[..., 0] for t in (out["film"], out["residual"]))
        if on_host:
            ok = np.isfinite(film).all(axis=-1) & np.isfinite(res).all(axis=-1)
            num, den = float((res[ok].astype(np.float64) ** 2).sum()), float((film[ok].astype(np.float64) ** 2).sum())
        else:
            import torch
            ok = torch.isfinite(film).all(dim=-1) & torch.isfinite(res).all(dim=-1)
            num, den = float((res[ok].double() ** 2).sum()), float((film[ok].double() ** 2).sum())
        out["residual_rel"] = float(np.sqrt(num / den)) if den > 0 else 0.0
    if view is not None and view is not False:
        out["picture"] = _view(scene, out["film"], **({} if view is True else view))
    return out


def _render_range_hip(scene, device):
    """render_to_noise's default renderer: the HIP path into fresh films on the scene's GPU (there is no CPU fallback)."""
    import torch
    if scene.device is None:
        scene.upload(device)
    dev = torch.device("cuda", scene.device)

    def renderer(begin, end, seed):
        with torch.cuda.device(dev):
            films = alloc_films(scene, dev)
            scene.render_into(*films, begin, end, seed, torch.cuda.current_stream(dev).cuda_stream)
        return films
    return renderer


def render_to_noise(scene, target, *, max_spp, chunk_spp=8, seed=1, device=0, mask=None, renderer=None, halves=False):
    """Renders until noise_estimate says the film is good enough, or until max_spp samples per element (even: both halves keep equal counts).  Two
    film sets: pair i renders the samples [2 i c, (2 i + 1) c) into A and [(2 i + 1) c, (2 i + 2) c) into B, c = chunk_spp (the last pair is
    shortened to what max_spp leaves); the RNG counter is (pixel, sample, stream), so A + B is the film one render of the same samples gives, up
    to the order of its additions.  After every pair one noise_estimate of A against B (on the device nothing but its record is downloaded);
    the loop stops when it is <= target.  `renderer(begin, end, seed) -> (value, weight, light)` (torch tensors, or numpy arrays for a CPU
    renderer) stands in for the HIP path in tests, as shard_renderer does in render_distributed.
    Returns ((value, weight, light) merged: A += B where the films are, samples per element, [(spp, estimate), ...] one entry per pair); with
    halves=True a fourth element, (A, B): copies of the two half-film sets as they stood before the merge, each of samples // 2 samples per element —
    what denoise() filters."""
    max_spp, c = int(max_spp), max(1, int(chunk_spp))
    if max_spp < 2 or max_spp % 2:
        raise ValueError(f"render_to_noise: an even max_spp >= 2 expected (two halves of equal size), got {max_spp}")
    render_range = renderer or _render_range_hip(scene, device)
    a = b = None
    done, history = 0, []
    while done < max_spp:
        h = min(c, (max_spp - done) // 2)
        parts = render_range(done, done + h, seed), render_range(done + h, done + 2 * h, seed)
        if a is None:
            a, b = parts
        else:
            for acc, part in zip((a, b), parts):
                for t, u in zip(acc, part):
                    t += u
        done += 2 * h
        history.append((done, noise_estimate(scene, a, b, done // 2, mask=mask)))
        if history[-1][1] <= target:
            break
    kept = tuple(tuple(t.copy() if isinstance(t, np.ndarray) else t.clone() for t in half) for half in (a, b)) if halves else None
    for t, u in zip(a, b):
        t += u
    return (a, done, history, kept) if halves else (a, done, history)


def render(scene, spp, seed=1, device=0, sample_begin=0):
    """Renders `spp` samples per element on one GPU; returns (value, weight, light) as numpy f64 arrays."""
    import torch
    if scene.device is None:
        scene.upload(device)
    dev = torch.device("cuda", scene.device)
    with torch.cuda.device(dev):
        value, weight, light = alloc_films(scene, dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        scene.render_into(value, weight, light, sample_begin, sample_begin + spp, seed, stream)
        torch.cuda.synchronize(dev)
    return value.cpu().numpy(), weight.cpu().numpy(), light.cpu().numpy()


def sensor_mask(scene, samples=None, seed=1, shapes=None, device=0):
    """The scene's by-geometry sensor mask (mask_t::create_mask, src/sensor/mask.cpp:28-66) computed on one GPU, as an H x W float32 numpy
    array — the alpha channel of imageio.write_masked.  Uploads the scene like render()."""
    import torch
    if scene.device is None:
        scene.upload(device)
    dev = torch.device("cuda", scene.device)
    with torch.cuda.device(dev):
        mask = scene.sensor_mask(samples, seed, shapes)
        torch.cuda.synchronize(dev)
    return mask.cpu().numpy()


def first_hit(scene, samples=0, seed=1, maps=("coverage", "depth", "position", "normal_geo", "normal_shading", "uv", "facing"), ids=("shape", "triangle"),
              device=0):
    """The scene's first-hit maps (Scene.first_hit: depth, position, normals, uv, facing, shape and triangle ids per pixel) computed on one
    GPU, as {name: numpy array} (ids: uint32, 0xFFFFFFFF without a hit).  Uploads the scene like render()."""
    import numpy as np
    import torch
    if scene.device is None:
        scene.upload(device)
    dev = torch.device("cuda", scene.device)
    with torch.cuda.device(dev):
        out = scene.first_hit(samples, seed, maps, ids)
        torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy().view(np.uint32) if v.dtype == torch.int32 else v.cpu().numpy() for k, v in out.items()}


def first_hit_material(scene, samples=0, seed=1, k=None, maps=("albedo", "specular", "opacity", "roughness", "emission"), ids=("material", "type"),
                       device=0):
    """The scene's first-hit material maps (Scene.first_hit_material: albedo, specular reflectance, opacity, roughness and emission per pixel and
    wavenumber, material index and leaf type) computed on one GPU, as {name: numpy array} (ids: uint32, 0xFFFFFFFF without a hit).  Uploads the
    scene like render()."""
    import torch
    if scene.device is None:
        scene.upload(device)
    dev = torch.device("cuda", scene.device)
    with torch.cuda.device(dev):
        out = scene.first_hit_material(samples, seed, k, maps, ids)
        torch.cuda.synchronize(dev)
    return {n: v.cpu().numpy().view(np.uint32) if v.dtype == torch.int32 else v.cpu().numpy() for n, v in out.items()}


def shard_samples(spp, rank, world):
    """Sample-index sharding: rank r renders [r*spp/world, (r+1)*spp/world)."""
    b = (spp * rank) // world
    e = (spp * (rank + 1)) // world
    return b, e


def _render_shard_hip(scene, begin, end, seed):
    """Default shard renderer: the HIP path on the rank's GPU (fails loudly without one: there is no CPU fallback)."""
    import torch
    if scene.device is None:
        raise RuntimeError("render_distributed: scene.upload(local_rank) first")
    dev = torch.device("cuda", scene.device)
    value, weight, light = alloc_films(scene, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    scene.render_into(value, weight, light, begin, end, seed, stream)
    return value, weight, light


def make_film_comm(device):
    """The C-ABI's RCCL communicator (wtgpu_comm_*: what a C++ host of the library uses) for the ranks of an initialised
    torch.distributed job: rank 0 creates the 128-byte id, torch.distributed carries it to the others (any transport would do)."""
    import torch.distributed as dist
    from .api import Comm
    rank, world = dist.get_rank(), dist.get_world_size()
    box = [Comm.unique_id() if rank == 0 else None]
    dist.broadcast_object_list(box, src=0)
    return Comm(world, rank, device, box[0])


def render_distributed(scene, spp, seed=1, reduce_dst=0, shard_renderer=None, comm=None):
    """One process per GPU (torch.distributed already initialised; backend nccl = RCCL on GPUs).  Each rank renders its
    sample shard of every pixel into its own film; the films are summed onto `reduce_dst`: with `comm` (make_film_comm) by the
    C-ABI's wtgpu_film_reduce (one group of three ncclReduce), otherwise by torch.distributed (GPU films go through the host when the
    backend is gloo: ranks that share a GPU, CPU tests).
    `shard_renderer(scene, begin, end, seed) -> (value, weight, light)` torch tensors is a seam for the CPU (gloo) tests of
    the sharding / reduction logic; the product path is the default (HIP)."""
    import torch
    import torch.distributed as dist
    rank, world = dist.get_rank(), dist.get_world_size()
    b, e = shard_samples(spp, rank, world)
    value, weight, light = (shard_renderer or _render_shard_hip)(scene, b, e, seed)
    if comm is not None:
        comm.film_reduce(value, weight, light, root=reduce_dst, stream=torch.cuda.current_stream(value.device).cuda_stream)
    else:
        via_host = value.is_cuda and dist.get_backend() == "gloo"
        if via_host:
            torch.cuda.synchronize(value.device)
            value, weight, light = value.cpu(), weight.cpu(), light.cpu()
        for t in (value, weight, light):
            dist.reduce(t, dst=reduce_dst, op=dist.ReduceOp.SUM)
    if value.is_cuda:
        torch.cuda.synchronize(value.device)
    if rank == reduce_dst:
        return value.cpu().numpy(), weight.cpu().numpy(), light.cpu().numpy()
    return None


def render_distributed_progressive(scene, spp, seed=1, reduce_dst=0, chunk_spp=8, on_partial=None, shard_renderer=None, comm=None):
    """render_distributed in chunks, with a PARTIAL film on `reduce_dst` after every chunk — what the reference's preview shows while a render
    runs (src/scene/render.cpp:306-368: the intermediate result is the merge of every worker's image), across ranks.  Every rank renders its
    shard [b, e) of the samples in chunks of `chunk_spp`; after each chunk the ranks reduce COPIES of their accumulators (the accumulators
    themselves stay per-rank: samples keep adding up locally, only the last reduce is the final film) and `on_partial(value, weight, light,
    samples_per_element_so_far)` is called on `reduce_dst` with the summed numpy films — e.g. to develop and push them to a TevPreview.  The
    chunk boundaries are the same on every rank (shards differ by at most one sample: ranks that run out render empty chunks), so the reduces
    match up without any other coordination.  Returns the final films on `reduce_dst` (None elsewhere)."""
    import torch
    import torch.distributed as dist
    rank, world = dist.get_rank(), dist.get_world_size()
    b, e = shard_samples(spp, rank, world)
    longest = max(shard_samples(spp, r, world)[1] - shard_samples(spp, r, world)[0] for r in range(world))
    acc = None
    done_here = 0
    result = None
    for c0 in range(0, max(longest, 1), max(1, chunk_spp)):
        cb, ce = min(e, b + c0), min(e, b + c0 + max(1, chunk_spp))
        if ce > cb or acc is None:
            part = (shard_renderer or _render_shard_hip)(scene, cb, ce, seed)     # (an empty range renders nothing and returns zero films)
            acc = part if acc is None else tuple(a.add_(p_) for a, p_ in zip(acc, part))
            done_here += ce - cb
        copies = tuple(t.clone() for t in acc)
        if comm is not None:
            comm.film_reduce(*copies, root=reduce_dst, stream=torch.cuda.current_stream(copies[0].device).cuda_stream)
        else:
            if copies[0].is_cuda and dist.get_backend() == "gloo":
                torch.cuda.synchronize(copies[0].device)
                copies = tuple(t.cpu() for t in copies)
            for t in copies:
                dist.reduce(t, dst=reduce_dst, op=dist.ReduceOp.SUM)
        if copies[0].is_cuda:
            torch.cuda.synchronize(copies[0].device)
        counts = torch.tensor([done_here], dtype=torch.int64)
        if dist.get_backend() == "nccl":
            counts = counts.to(copies[0].device)
        dist.reduce(counts, dst=reduce_dst, op=dist.ReduceOp.SUM)
        if rank == reduce_dst:
            result = tuple(t.cpu().numpy() for t in copies)
            if on_partial is not None:
                on_partial(*result, int(counts.item()))
    return result if rank == reduce_dst else None
