"""Headless batch driver of the denovo3D parameter sweep.

The reference's README lists a ``denovo3DBatch`` command (README.md:27) but ships no module for it;
its interactive counterpart is ``run_denovo3D_reconstruction`` (src/helicon/webApps/denovo3D/app.py:
2286-2452), whose grid construction (``np.arange(min, max + step/2, step)`` axes, twist-major
``itertools.product``, wrap/round of the twist, skipped pairs) and result ordering (scores sorted
descending, app.py:2521-2523) this driver reproduces without the Shiny UI.

    python -m helicon_amd.denovo3DBatch image.npy --apix 2.0 --twist 25 33 0.2 --rise 8 13 0.2 \\
           --csym 1 --out scores.npz [--mask mask.npy] [--no-log] [--device 0] [--top 10] \
           [--cutoff-res 10 10 --spectrum-size 256 256] [--spectrum-high-pass 0.05] [--spectrum-low-pass 0.3] [--phase-weight 0.5] \
           [--rescore 20 --tube-diameter 120 --interpolation linear [--half-map-fsc 1]]

``--rescore K`` runs the reference's own scorer — the sparse least-squares reconstruction of pipeline.py:84-496,
``process_one_task(..., algorithm={"scorer": "lsq"})`` — on the sweep's K best candidates of every image, from a
thread pool like the app's (app.py:2473-2476), and reports them in the order of that score.

``--rescore K --half-map-fsc {1,2}`` also solves the two half-data problems of every rescored candidate (the scorer's
``fsc_test``: 1 = random halves of the pixels, 2 = even / odd), symmetrises both half maps onto a cube and adds their Fourier
shell correlation to the record (``fsc``, ``fsc_resolution_0143``, ``fsc_resolution_05``; ``helicon_amd.fsc.half_map_fsc``,
all candidates of a box group in one batched call) and ``rescored_fsc`` to ``--out``.  It needs ``--tilt 0 --psi 0``.

``--cutoff-res Y X`` (Angstrom) and ``--spectrum-size NY NX`` score on the Fourier-zoomed power spectrum
``compute_power_spectra(image, apix, cutoff_res=(Y, X), output_size=(NY, NX))`` (transforms.py:663-713, 771-820) of the
image and of every candidate: the spectrum stops at that resolution instead of Nyquist and NY x NX samples cover it.  A
``--mask`` file then has the shape NY x NX.  Either flag may be given alone (the other keeps its default: Nyquist, the
image's shape).

``--spectrum-low-pass F`` / ``--spectrum-high-pass F`` score on the filtered spectrum ``compute_power_spectra(...,
low_pass_fraction=F, high_pass_fraction=F)`` (transforms.py:811-816): the Gaussian low / high pass of the spectrum image, as
fractions of its Nyquist radius; a high pass removes the spectrum's smooth radial fall-off.  A fraction outside (0, 1) is
off.  They combine with the zoom flags and with ``--mask``, which keeps the shape of the scored spectrum.

``--phase-weight W`` scores ``(1 - W) * amplitude Pearson + W * phase score``: the phase score compares the phase difference
across the meridian (``compute_phase_difference_across_meridian``, transforms.py:823-842) of the image and of every
candidate, which tells an even Bessel order from an odd one where the amplitudes cannot.  The helix must be centred on the
image's middle row (or ``--dy`` must say where it is).  W in (0, 1]; 0 is off.  It combines with the zoom flags and is
refused together with the spectrum filter flags.  With the flag on, the report and ``--out`` record ``phase_weight``.

``--from-map TWIST RISE CSYM`` reads ``image`` as a 3-D map instead (``.mrc`` / ``.map`` / ``.npy``, ``--apix`` its voxel
size) and builds the input image as the app does for a map (app.py:1780-1829): the map is symmetrised with the given
twist, rise and Csym, resampled to ``--output-size`` at ``--output-apix`` with ``--axial-rotation`` / ``--output-tilt``
(``symmetrize_transform_map``), projected along x, and ``--noise`` times its foreground standard deviation of Gaussian noise
is added.  The sweep and ``--rescore`` then run on that image at the output pixel size (for a map whose symmetry is not
known, ``python -m helicon_amd.symmetry_search`` finds it: its report's ``best`` is what TWIST RISE CSYM take):

    python -m helicon_amd.denovo3DBatch emd.map --from-map 29.4 4.75 1 --output-apix 5 --twist 28 31 0.2 --rise 4 6 0.1 \
           --seed 0 --save-projection proj.npy

Images are ``.npy`` arrays or MRC files/stacks (``[ny, nx]`` or ``[S, ny, nx]``, helical axis along x; square
power-of-two sides 32…1024 run the tuned kernels, any other size in 8…1024 the runtime-sized ones); ``--index``
picks slices of a stack like ``read_image_2d`` (io_mrc.py:71-100).
"""
from __future__ import annotations

import argparse
import json
import sys

import numpy as np

from .denovo3D import sweep
from .grid import filter_spec, phase_spec, sweep_axis, zoom_spec


def add_args(parser: argparse.ArgumentParser) -> argparse.ArgumentParser:
    parser.add_argument("image", help=".npy / .mrc / .mrcs file with one [N, N] image or a stack [S, N, N]")
    parser.add_argument("--index", type=int, nargs="*", default=None, help="slices of the stack to use (default: all)")
    parser.add_argument("--apix", type=float, default=None, help="pixel size, Angstrom (default: the MRC header's)")
    parser.add_argument("--twist", type=float, nargs=3, metavar=("MIN", "MAX", "STEP"), required=True)
    parser.add_argument("--rise", type=float, nargs=3, metavar=("MIN", "MAX", "STEP"), required=True)
    parser.add_argument("--csym", type=int, nargs="+", default=[1])
    parser.add_argument("--helical-diameter", type=float, default=None, help="Angstrom (default 0.4 * ny * apix)")
    parser.add_argument("--ball-radius", type=float, default=None, help="Angstrom (default 2 * apix)")
    parser.add_argument("--rot", type=float, default=0.0)
    parser.add_argument("--tilt", type=float, default=0.0)
    parser.add_argument("--psi", type=float, default=0.0)
    parser.add_argument("--dy", type=float, default=0.0)
    parser.add_argument("--mask", default=None, help=".npy boolean mask on the fftshifted plane (default: radial band)")
    parser.add_argument("--no-log", action="store_true", help="correlate |F| instead of log1p|F|")
    parser.add_argument("--cutoff-res", type=float, nargs=2, metavar=("Y", "X"), default=None,
                        help="score on spectra that stop at this resolution (Angstrom) instead of Nyquist (compute_power_spectra's cutoff_res)")
    parser.add_argument("--spectrum-size", type=int, nargs=2, metavar=("NY", "NX"), default=None,
                        help="samples of the scored spectrum (compute_power_spectra's output_size; default: the image's shape)")
    parser.add_argument("--spectrum-low-pass", type=float, default=0.0, metavar="F",
                        help="Gaussian low pass of the scored spectrum image (compute_power_spectra's low_pass_fraction; outside (0, 1): off)")
    parser.add_argument("--spectrum-high-pass", type=float, default=0.0, metavar="F",
                        help="Gaussian high pass of the scored spectrum image (compute_power_spectra's high_pass_fraction; outside (0, 1): off)")
    parser.add_argument("--phase-weight", type=float, default=0.0, metavar="W",
                        help="weight in [0, 1] of the phase score across the meridian in the score (0: amplitudes alone); not with the spectrum filter flags")
    parser.add_argument("--device", type=int, default=0)
    parser.add_argument("--top", type=int, default=10, help="how many best candidates to print per image")
    parser.add_argument("--out", default=None, help=".npz with scores[S, C, T, R], twists, rises, csyms")
    parser.add_argument("--rescore", type=int, default=0, help="re-score this many best candidates per image with the least-squares scorer")
    parser.add_argument("--tube-diameter", type=float, default=None, help="Angstrom, for --rescore (default 0.8 * ny * apix)")
    parser.add_argument("--interpolation", choices=("nn", "linear"), default="linear",
                        help="for --rescore: the projector of the least-squares scorer — linear (trilinear, the reference app's "
                             "default, app.py:577-585) or nn (nearest neighbour); both set up and solve all candidates together "
                             "on the device.  The two give different scores for the same candidate.")
    parser.add_argument("--model", choices=("lsq", "elasticnet", "lasso", "ridge", "lreg"), default="lsq",
                        help="for --rescore: the solver of the least-squares scorer (solver_linear_regression.py:205-342; the "
                             "reference app's default is elasticnet, app.py:553-559); --map-out's map is solved with it too.  A model other than lsq "
                             "needs --tilt 0 --psi 0.")
    parser.add_argument("--l1-ratio", type=float, default=0.5, help="for --rescore --model elasticnet")
    parser.add_argument("--alpha", type=float, default=None, help="for --rescore with a model: its regularisation strength "
                        "(default: the model's own — 1e-4 for elasticnet and lasso, 1 for ridge)")
    parser.add_argument("--threads", type=int, default=8, help="for --rescore")
    parser.add_argument("--half-map-fsc", type=int, choices=(1, 2), default=0, metavar="{1,2}",
                        help="for --rescore: also solve the two half-data problems (the scorer's fsc_test: 1 random halves, 2 even / odd "
                             "pixels) and report the Fourier shell correlation of the symmetrised half maps; needs --tilt 0 --psi 0")
    parser.add_argument("--map-out", default=None, help="for --rescore: write the best candidate's helically symmetrised map of every "
                        "image to <map-out>_<image>.mrc (the app's map download, app.py:1267-1287)")
    g = parser.add_argument_group("map input (app.py:1780-1829)")
    g.add_argument("--from-map", type=float, nargs=3, metavar=("TWIST", "RISE", "CSYM"), default=None,
                   help="read IMAGE as a 3-D map (.mrc / .map / .npy) with this helical symmetry and sweep its projection")
    g.add_argument("--output-apix", type=float, default=5.0, help="pixel size of the projection, Angstrom (app.py:312)")
    g.add_argument("--output-size", type=int, nargs=2, metavar=("LENGTH", "WIDTH"), default=None,
                   help="the resampled map is LENGTH x WIDTH x WIDTH voxels (default: the app's rule, app.py:266-273)")
    g.add_argument("--axial-rotation", type=float, default=0.0, help="degrees, about the helical axis")
    g.add_argument("--output-tilt", type=float, default=0.0, help="degrees, out of plane")
    g.add_argument("--noise", type=float, default=1.0,
                   help="Gaussian noise, in units of the projection's foreground standard deviation (app.py:359, 1818-1821)")
    g.add_argument("--seed", type=int, default=None, help="seed of NumPy's global generator before the noise is drawn")
    g.add_argument("--save-projection", default=None, help="write the image that is swept (.npy or .mrc)")
    return parser


def default_output_size(nx, apix, output_apix, twist, rise) -> tuple[int, int]:
    """app.py:266-273 with the output pixel size in place of its literal 5: width = int(nx apix / output_apix) // 4 * 4,
    length = int(round(0.5 pitch / output_apix)) // 4 * 4 with pitch = 360 rise / |twist| (twice the width when the
    pitch is undefined, twist = 0)."""
    width = int(nx * apix / output_apix) // 4 * 4
    if twist == 0:
        return width * 2, width
    pitch = 360.0 * rise / abs(twist)
    return int(round(0.5 * pitch / output_apix)) // 4 * 4, width


def map_to_image(vol, apix, twist, rise, csym, output_apix, output_size, axial_rotation=0.0, tilt=0.0, noise=1.0, device=0):
    """The app's image of a map (app.py:1780-1829): ``symmetrize_transform_map`` onto LENGTH x WIDTH x WIDTH voxels of
    output_apix, the sum along x transposed and flipped left-right (``xyz[0].T[:, ::-1]``: rows across the helix, columns
    along it), then, for noise > 0, N(0, (noise sigma)^2) from NumPy's global generator with sigma the standard deviation of
    the pixels above 1e-3.  float32."""
    from .denovo3D import generate_xyz_projections, symmetrize_transform_map

    length, width = (int(v) for v in output_size)
    if length < 1 or width < 1:
        raise ValueError(f"the output size must be positive; got length {length}, width {width}")
    m = symmetrize_transform_map(vol, apix, twist, rise, int(csym), 1.0, (length, width, width), output_apix, axial_rotation,
                                 tilt, device=device)
    proj = np.ascontiguousarray(generate_xyz_projections(m, device=device)[0].T[:, ::-1], dtype=np.float32)
    if noise > 0:
        fg = proj[proj > 1e-3]
        if fg.size == 0:
            raise ValueError("the projection has no pixel above 1e-3: there is no foreground to scale the noise by")
        proj += np.random.normal(scale=np.std(fg) * noise, size=proj.shape)   # in place on float32, as app.py:1820
    return proj


def _map_input(args):
    """--from-map: the map, its voxel size and the projection that is swept (args.apix becomes the output pixel size)."""
    twist, rise, csym = args.from_map
    if csym != int(csym) or csym < 1:
        raise SystemExit(f"--from-map: CSYM must be a positive integer; got {csym}")
    if not rise > 0:
        raise SystemExit(f"--from-map: RISE must be > 0; got {rise}")
    if not args.output_apix > 0:
        raise SystemExit(f"--output-apix must be > 0; got {args.output_apix}")
    if args.index:
        raise SystemExit("--index selects slices of a 2-D stack; it does not apply to --from-map")
    if str(args.image).lower().endswith((".mrc", ".mrcs", ".map")):
        from .mrc import read_mrc

        vol, header_apix = read_mrc(args.image)
        if args.apix is None:
            args.apix = header_apix
    else:
        vol = np.load(args.image)
    if vol.ndim != 3:
        raise SystemExit(f"--from-map needs a 3-D map; {args.image} has shape {vol.shape}")
    if not args.apix or args.apix <= 0:
        raise SystemExit("--apix is required (the map carries no voxel size)")
    size = tuple(args.output_size) if args.output_size else default_output_size(vol.shape[2], args.apix, args.output_apix, twist, rise)
    if min(size) < 8 or max(size) > 1024:
        raise SystemExit(f"the output size (length {size[0]}, width {size[1]}) must lie in [8, 1024]: set --output-size")
    if args.seed is not None:
        np.random.seed(args.seed)
    proj = map_to_image(vol, args.apix, twist, rise, int(csym), args.output_apix, size, args.axial_rotation, args.output_tilt,
                        args.noise, args.device)
    if args.save_projection:
        if str(args.save_projection).lower().endswith((".mrc", ".mrcs", ".map")):
            from .mrc import write_mrc

            write_mrc(args.save_projection, proj, args.output_apix)
        else:
            np.save(args.save_projection, proj)
    info = dict(path=str(args.image), shape=[int(v) for v in vol.shape], apix=float(args.apix), twist=float(twist), rise=float(rise),
                csym=int(csym), output_apix=float(args.output_apix), output_size=[int(v) for v in size],
                axial_rotation=float(args.axial_rotation), tilt=float(args.output_tilt), noise=float(args.noise), seed=args.seed,
                projection_shape=[int(v) for v in proj.shape])
    args.apix = args.output_apix
    return proj[None], info


def rescore_algorithm(args) -> dict:
    """The ``algorithm`` dict of the least-squares scorer from --model / --l1-ratio / --alpha (lsq_reconstruct's keys)."""
    model = getattr(args, "model", "lsq")
    alg = {"model": model}
    if model == "elasticnet":
        alg["l1_ratio"] = float(args.l1_ratio)
    if model != "lsq" and getattr(args, "alpha", None) is not None:
        alg["alpha"] = float(args.alpha)
    return alg


def run(args) -> dict:
    if getattr(args, "model", "lsq") != "lsq" and (args.tilt != 0 or args.psi != 0):
        raise SystemExit(f"--model {args.model} needs --tilt 0 --psi 0: the scikit-learn models run in the group solver, "
                         "whose products have no tilted form")
    half_fsc = int(getattr(args, "half_map_fsc", 0) or 0)
    if half_fsc and args.rescore > 0 and (args.tilt != 0 or args.psi != 0):
        raise SystemExit("--half-map-fsc needs --tilt 0 --psi 0: with a tilt the rescoring goes through process_one_task one "
                         "candidate at a time, which returns no half maps")
    map_info = None
    if getattr(args, "from_map", None) is not None:
        images, map_info = _map_input(args)
    elif str(args.image).lower().endswith((".mrc", ".mrcs", ".map")):
        from .mrc import read_mrc

        images, header_apix = read_mrc(args.image)
        if args.apix is None:
            args.apix = header_apix
    else:
        images = np.load(args.image)
    if not args.apix or args.apix <= 0:
        raise SystemExit("--apix is required (the input carries no pixel size)")
    if images.ndim == 2:
        images = images[None]
    if args.index and map_info is None:
        images = images[np.asarray(args.index)]
    images = np.ascontiguousarray(images, dtype=np.float32)
    n = images.shape[-2]  # rows: the lattice has to fit across the helical axis (utils.py:88)
    twists = sweep_axis(*args.twist)
    rises = sweep_axis(*args.rise)
    mask = np.load(args.mask) if args.mask else None
    cutoff_res = tuple(args.cutoff_res) if getattr(args, "cutoff_res", None) else None
    spectrum_size = tuple(args.spectrum_size) if getattr(args, "spectrum_size", None) else None
    try:
        zoom = zoom_spec(images.shape[-2:], args.apix, cutoff_res, spectrum_size)
    except ValueError as e:
        raise SystemExit(f"--cutoff-res / --spectrum-size: {e}")
    plane = (zoom[0], zoom[1]) if zoom else tuple(int(v) for v in images.shape[-2:])
    if mask is not None and tuple(mask.shape) != plane:
        raise SystemExit(f"--mask {args.mask} has shape {tuple(mask.shape)}; the scored spectrum is {plane[0]} x {plane[1]}" +
                         (" (--spectrum-size / --cutoff-res)" if zoom else " (the image's shape)"))
    try:
        filt = filter_spec(getattr(args, "spectrum_low_pass", 0.0), getattr(args, "spectrum_high_pass", 0.0))
    except ValueError as e:
        raise SystemExit(f"--spectrum-low-pass / --spectrum-high-pass: {e}")
    filter_kw = dict(low_pass_fraction=filt[0], high_pass_fraction=filt[1]) if filt else {}   # off: sweep() is called as without the flags
    try:
        phase = phase_spec(getattr(args, "phase_weight", 0.0))
    except ValueError as e:
        raise SystemExit(f"--phase-weight: {e}")
    if phase is not None and filt:
        raise SystemExit("--phase-weight does not combine with --spectrum-low-pass / --spectrum-high-pass: the phase score reads the unfiltered transform")
    if phase is not None:
        filter_kw["phase_weight"] = phase
    res = sweep(
        images, twists, rises, tuple(args.csym), apix=args.apix,
        helical_diameter=args.helical_diameter if args.helical_diameter is not None else 0.4 * n * args.apix,
        ball_radius=args.ball_radius if args.ball_radius is not None else 2.0 * args.apix,
        mask=mask, log=not args.no_log, rot=args.rot, tilt=args.tilt, psi=args.psi, dy=args.dy, device=args.device,
        cutoff_res=cutoff_res, output_size=spectrum_size, **filter_kw,
    )
    report = {"n_candidates": int(len(res.grid)), "n_skipped": int((~res.grid.valid).sum()), "images": []}
    # the sampling that was scored (the defaults written out: Nyquist, the image's shape)
    report["cutoff_res"] = [float(zoom[2]), float(zoom[3])] if zoom else [2.0 * args.apix, 2.0 * args.apix]
    report["spectrum_size"] = [int(plane[0]), int(plane[1])]
    report["spectrum_filter"] = [float(filt[0]), float(filt[1])] if filt else [0.0, 0.0]   # (low pass, high pass); 0 = off
    if phase is not None:   # (off: the report and the file are what they are without the flag)
        report["phase_weight"] = float(phase)
    if map_info is not None:
        report["map"] = map_info
    flat = res.scores.reshape(res.scores.shape[0], -1)
    for s in range(flat.shape[0]):
        order = np.argsort(-flat[s], kind="stable")[: args.top]  # score descending, like app.py:2521-2523
        report["images"].append({
            "index": s,
            "best": dict(zip(("twist", "rise", "csym", "score"), res.best[s])),
            "top": [dict(twist=float(res.grid.params[g, 0]), rise=float(res.grid.params[g, 1]),
                         csym=int(res.grid.params[g, 2]), score=float(flat[s, g])) for g in order],
        })
    if args.rescore > 0:
        for s in range(flat.shape[0]):
            report["images"][s]["rescored"] = rescore(images[s], report["images"][s]["top"][: args.rescore], args)
            if args.map_out and report["images"][s]["rescored"]:
                report["images"][s]["map"] = write_best_map(images[s], report["images"][s]["rescored"][0], args, f"{args.map_out}_{s}.mrc")
    if args.rescore > 0:
        report["rescore_interpolation"] = args.interpolation
        report["rescore_model"] = rescore_algorithm(args)
        print(f"denovo3DBatch --rescore: least-squares scorer with interpolation = {args.interpolation}, "
              f"model = {report['rescore_model']['model']}", file=sys.stderr)
    if args.out:
        extra = {}
        if args.rescore > 0:
            alg = report["rescore_model"]
            extra = dict(rescore_interpolation=np.asarray(args.interpolation), rescore_model=np.asarray(alg["model"]),
                         rescore_l1_ratio=np.asarray(alg.get("l1_ratio", np.nan)), rescore_alpha=np.asarray(alg.get("alpha", np.nan)),
                         rescored=np.asarray([[[r["twist"], r["rise"], r["csym"], r["sweep_score"],
                                                np.nan if r["lsq_score"] is None else r["lsq_score"]]
                                               for r in im.get("rescored", [])] for im in report["images"]], dtype=np.float64))
            if half_fsc and all("fsc" in r for im in report["images"] for r in im.get("rescored", [])):   # [image][rescored candidate][shell][saxis, fsc] and the two resolutions, in the order of `rescored`
                extra["rescored_fsc"] = np.asarray([[r["fsc"] for r in im.get("rescored", [])] for im in report["images"]], dtype=np.float64)
                extra["rescored_fsc_resolution"] = np.asarray([[[r["fsc_resolution_0143"], r["fsc_resolution_05"]]
                                                                for r in im.get("rescored", [])] for im in report["images"]], dtype=np.float64)
        if "phase_weight" in report:
            extra["phase_weight"] = np.asarray(report["phase_weight"])
        np.savez_compressed(args.out, scores=res.scores, twists=twists, rises=rises, csyms=np.asarray(args.csym),
                            params=res.grid.params, valid=res.grid.valid, cutoff_res=np.asarray(report["cutoff_res"]),
                            spectrum_size=np.asarray(report["spectrum_size"]), spectrum_filter=np.asarray(report["spectrum_filter"]), **extra)
    return report


def rescore(image, candidates, args) -> list:
    """The least-squares scorer on a list of sweep candidates (dicts with twist, rise, csym, score), best first.

    With tilt = psi = 0 (the reference app's own setting, app.py:2344-2346) the candidates go through
    ``lsq_reconstruct_batch`` with either projector: they are grouped by reconstruction box (the reference derives the box
    length from the candidate's rise, pipeline.py:259-266, 319-331) and every group is set up and solved on the device at
    once — scores only, the display products of ``process_one_task`` (symmetrised map, projections) are made for the one
    map ``--map-out`` asks for.  With tilt / psi every candidate is one ``process_one_task`` call from a thread pool, like
    the reference's driver (app.py:2473-2476).  Candidates with |twist| < 0.01 degree are skipped as the reference's
    driver skips them (app.py:2389-2393).  Every record names the projector: the two give different scores."""
    ny, nx = image.shape
    tube_d = args.tube_diameter if args.tube_diameter is not None else 0.8 * ny * args.apix
    usable = [c for c in candidates if abs(c["twist"]) >= 0.01]   # the reference skips such pairs (app.py:2389-2393)
    if len(usable) < len(candidates):
        print(f"denovo3DBatch --rescore: {len(candidates) - len(usable)} candidate(s) with |twist| < 0.01 degree skipped "
              "(the least-squares scorer divides by the twist)", file=sys.stderr)
        candidates = usable
    if not candidates:
        return []
    if args.tilt == 0 and args.psi == 0:   # the group solver (tilt / psi: process_one_task below, one call per candidate)
        from .denovo3D import _prepare_task_image, lsq_box
        from .solver import lsq_reconstruct_batch

        if not np.std(image):   # pipeline.py:214-218
            return [dict(twist=c["twist"], rise=c["rise"], csym=c["csym"], sweep_score=c["score"], lsq_score=None) for c in candidates]
        img = np.asarray(_prepare_task_image(image, args.apix, 0, 0, None, tube_d, args.device))
        groups = {}
        for k, c in enumerate(candidates):
            box = lsq_box(ny, nx, args.apix, c["rise"], (c["rise"], c["rise"]), (0, 0), args.apix, -1, tube_d, 0, -1, 1, 0)
            groups.setdefault(box, []).append(k)
        scores = [None] * len(candidates)
        half_fsc = int(getattr(args, "half_map_fsc", 0) or 0)
        fsc_of = [None] * len(candidates)
        for (a3, d2, l2, d3, d3_inner, l3, oversample), members in groups.items():
            res = lsq_reconstruct_batch(img, args.apix / a3, [(candidates[k]["twist"], candidates[k]["rise"] / a3, candidates[k]["csym"])
                                                             for k in members],
                                        reconstruct_diameter_3d_inner_pixel=d3_inner, reconstruct_diameter_2d_pixel=d2,
                                        reconstruct_diameter_3d_pixel=d3, reconstruct_length_2d_pixel=l2, reconstruct_length_3d_pixel=l3,
                                        sym_oversample=oversample, fsc_test=half_fsc, return_3d=bool(half_fsc), device=args.device,
                                        streams=max(1, args.threads), interpolation=args.interpolation, algorithm=rescore_algorithm(args))
            for k, (_, sc) in zip(members, res):
                scores[k] = sc
            if half_fsc:   # every half map of the group symmetrised onto its cube, then one batched correlation
                from .fsc import half_map_fsc_batch

                curves = half_map_fsc_batch([maps[1] for maps, _ in res], [maps[2] for maps, _ in res], a3,
                                            [(candidates[k]["twist"], candidates[k]["rise"], candidates[k]["csym"]) for k in members],
                                            device=args.device)
                for k, (curve, resolution) in zip(members, curves):
                    fsc_of[k] = dict(fsc_resolution_0143=resolution["0.143"], fsc_resolution_05=resolution["0.5"], fsc=curve.tolist())
        got = [dict(twist=c["twist"], rise=c["rise"], csym=c["csym"], sweep_score=c["score"], lsq_score=float(scores[k]),
                    interpolation=args.interpolation, **(fsc_of[k] or {})) for k, c in enumerate(candidates)]
        return sorted(got, key=lambda r: -r["lsq_score"])

    from concurrent.futures import ThreadPoolExecutor

    from .denovo3D import process_one_task

    def one(c):
        # the 36 positional arguments of pipeline.py:84-121 (no rescale: target_apix2d = apix; voxel size = pixel size)
        out = process_one_task(0, 1, image, "", 1, c["twist"], c["rise"], (c["rise"], c["rise"]), c["csym"], 0.0, (0, 0),
                               0.0, 0, 0.0, 0, args.apix, "", 0, 0, 0, 0, args.apix, -1, -1, -1, tube_d, 0, -1, 1,
                               args.interpolation, 0, 0, "cosine", dict(rescore_algorithm(args), scorer="lsq", device=args.device), 0, 1)
        return dict(twist=c["twist"], rise=c["rise"], csym=c["csym"], sweep_score=c["score"],
                    lsq_score=None if out is None else float(out[0]), interpolation=args.interpolation)

    with ThreadPoolExecutor(max_workers=max(1, args.threads)) as pool:
        got = list(pool.map(one, candidates))
    return sorted(got, key=lambda r: -(r["lsq_score"] if r["lsq_score"] is not None else -np.inf))


def write_best_map(image, best, args, path) -> str:
    """app.py:1267-1287: the candidate's least-squares map, helically symmetrised onto the input's grid
    (new_size = (nx, ny, ny) at the input's pixel size), as an MRC file."""
    from .denovo3D import apply_helical_symmetry, process_one_task
    from .mrc import write_mrc

    ny, nx = image.shape
    tube_d = args.tube_diameter if args.tube_diameter is not None else 0.8 * ny * args.apix
    out = process_one_task(0, 1, image, "", 1, best["twist"], best["rise"], (best["rise"], best["rise"]), best["csym"], 0.0, (0, 0),
                           0.0, 0, 0.0, 0, args.apix, "", 0, 0, 0, 0, args.apix, -1, -1, -1, tube_d, 0, -1, 1, args.interpolation,
                           0, 1, "cosine", dict(rescore_algorithm(args), scorer="lsq", device=args.device), 0, 1)
    rec3d, apix3d = out[1][3][0], out[2][3]
    vol = apply_helical_symmetry(rec3d, apix3d, best["twist"], best["rise"], best["csym"], 1.0, (nx, ny, ny), args.apix,
                                 device=args.device).astype(np.float32)
    write_mrc(path, vol, args.apix)
    return str(path)


def main(argv=None) -> int:
    args = add_args(argparse.ArgumentParser(prog="denovo3DBatch", description=__doc__.split("\n\n")[0])).parse_args(argv)
    json.dump(run(args), sys.stdout, indent=1)
    sys.stdout.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
