"""`python -m grav1synth_amd diff SOURCE [DENOISED | --denoise] -o OUT [-y] [-f FILTERS]` -- the front door of the path
(and `estimate`, `render`, `denoise`, `measure`, `check`).

The `diff` command of the reference (Commands::Diff, /root/reference/src/main.rs:347-533, arguments :846-870) for .y4m
inputs, around g1s_diff_y4m_files_filtered: the same refusals in the same order, with the same texts, and like the
reference every refusal is a logged line and a normal exit --

  * an input path equal to the output path              (src/main.rs:354-360)
  * source path equal to denoised path                  (src/main.rs:362-368)
  * a filter chain that does not parse                  (src/main.rs:370-380: "Invalid filter chain: {e}")
  * an existing output without -y and without a "yes"   (src/main.rs:382-394)

-- then the frame-pair loop, finish, the table (src/main.rs:414-529) and the two closing lines (:531-532)."""
from __future__ import annotations

import argparse
import logging
import os
import sys
from typing import List, Optional

log = logging.getLogger("grav1synth")

SAME_AS_OUTPUT = ("Input and output paths are the same. This is probably a typo, because this would overwrite your "
                  "input. Exiting.")
SAME_INPUTS = ("Source and denoised paths are the same. This is probably a typo, because this would always compute an "
               "empty diff. Exiting.")
NOT_OVERWRITING = "Not overwriting existing file. Exiting."
SAME_OUTPUTS = "--temporal and -o name the same file: the two reports would overwrite each other. Exiting."
SAME_CROSS_OUTPUT = "--cross and -o name the same file: the two reports would overwrite each other. Exiting."
SAME_CROSS_TEMPORAL = "--cross and --temporal name the same file: the two reports would overwrite each other. Exiting."
SAME_SCALES_OUTPUT = "--scales and -o name the same file: the two reports would overwrite each other. Exiting."
SAME_SCALES_TEMPORAL = "--scales and --temporal name the same file: the two reports would overwrite each other. Exiting."
SAME_SCALES_CROSS = "--scales and --cross name the same file: the two reports would overwrite each other. Exiting."
CROSS_NEEDS_CHROMA = "--cross compares chroma with luma: the clip has no chroma planes"
SAME_TABLE = "--table and --lags cannot be the same file as the source, the output, a report or each other. Exiting."
TABLE_BAD_LAG = "--table-lag must be 1, 2 or 3. Exiting."
TABLE_NEEDS_FLAG = "--table-lag, --lags, --profile-frames and --levels-min-count say how --table is made: they need it. Exiting."
TABLE_NEEDS_TWO = "a table needs two frames. Exiting."
SAME_LEVELS = "--levels and -o name the same file: the two outputs would overwrite each other. Exiting."
NO_DENOISED = "Neither a DENOISED file nor --denoise was given: there is nothing to compare the source with. Exiting."
BOTH_DENOISED = "--denoise makes the denoised clip on the device: it does not combine with a DENOISED file. Exiting."
DENOISE_NO_FILTERS = "--denoise does not combine with --filters (the denoiser runs on the source as it is read). Exiting."
DENOISE_ONE_DEVICE = "--denoise does not combine with --gpus / --devices (one denoiser, one generator, one device). Exiting."
BAD_TEMPORAL_RADIUS = "--temporal-radius must be 0..3 (frames before and after the one in hand). Exiting."
BAD_MOTION_RANGE = "--motion-range must be even and 0..64 (samples a tile may move between two frames). Exiting."
MOTION_NEEDS_TEMPORAL = "--motion-range moves the neighbour frames of --temporal-radius: it needs a temporal radius above 0. Exiting."
BAD_COARSE_LEVELS = "--coarse-levels must be 0..2 (box means of the frame that are filtered as well). Exiting."
BAD_COARSE_RATIO = "--coarse-ratio must be 0.0625..4 (a coarse level's strength over that of the level above it; 0 = 1). Exiting."
RATIO_NEEDS_LEVELS = "--coarse-ratio scales the strength of --coarse-levels: it needs a level above 0. Exiting."
KEEP_NEEDS_DENOISE = "--keep-denoised writes the clip --denoise makes: it needs --denoise. Exiting."
PRIOR_NEEDS_TABLE = "--prior-range and --prior-segment say how --grain-prior is used: they need --grain-prior. Exiting."
PRIOR_12_BIT = ("--grain-prior filters luma in a 12-bit domain: a 12-bit input has no headroom there (8 and 10 bits are "
                "supported). Exiting.")
AUTO_PRIOR_AND_TABLE = "--auto-prior measures the prior that --grain-prior would read from a table: they do not combine. Exiting."
AUTO_STRENGTH_AND_STRENGTH = "--auto-strength measures what --strength and --chroma-strength would set: they do not combine. Exiting."
AUTO_NEEDS_FLAG = "--profile-frames and --levels-min-count say how --auto-prior and --auto-strength measure: they need one of them. Exiting."
AUTO_TEMPORAL_NEEDS_FLAG = "--auto-temporal says how --auto-prior and --auto-strength measure: it needs one of them. Exiting."
AUTO_TEMPORAL_NEEDS_TWO = "--auto-temporal measures the difference of consecutive frames: --profile-frames 1 leaves none. Exiting."
SAME_LEVELS_TEMPORAL = "--levels-temporal cannot be the same file as the output or --levels. Exiting."
AUTO_BAD_NUMBER = "--profile-frames and --levels-min-count must not be negative. Exiting."
AUTO_NEEDS_FILE = "--auto-prior and --auto-strength read the input twice: %s is not a regular file. Exiting."
PRIOR_BAD_TABLE = "Invalid grain prior: %s. Exiting."
CHROMA_PRIOR_NEEDS_PRIOR = "--chroma-prior extends the job's grain prior to chroma: it needs --grain-prior or --auto-prior. Exiting."
CHROMA_PRIOR_NEEDS_JOINT = "--chroma-prior reads the luma under every chroma sample: it needs --joint-chroma. Exiting."
CHROMA_PRIOR_BAD_RANGE = "--chroma-prior takes a --prior-range of 1..8. Exiting."
PRIOR_BAD_SEGMENT = "--prior-segment %d is not in the grain prior (%d segments). Exiting."


def _confirm(prompt: str) -> bool:
    """dialoguer::Confirm::interact()?: y / n on the terminal.  Without a terminal dialoguer returns an error, which the
    reference's `?` turns into a non-zero exit (src/main.rs:382-394): the same here (main() reports it and returns 1)."""
    if not sys.stdin.isatty():
        raise OSError("IO error: not a terminal")
    try:
        return input(f"{prompt} [y/n] ").strip().lower() in ("y", "yes")
    except EOFError:
        raise OSError("IO error: unexpected end of input")


def _same_path(a: str, b: str) -> bool:
    """`PathBuf == PathBuf` as the reference compares its arguments (src/main.rs:354, :362): component by component, so
    repeated separators, a trailing separator and `.` components inside the path do not matter (a leading `./` and `..` do:
    std::path::Path::components)."""
    def components(p: str):
        parts = p.split("/")
        out = ["/"] if p.startswith("/") else []
        for i, c in enumerate(parts):
            if c == "" or (c == "." and (i > 0 or p.startswith("/"))):
                continue
            out.append(c)
        return out
    return components(a) == components(b)


def _add_denoise_parameters(p: argparse.ArgumentParser) -> None:
    """The filter's parameters, shared by `denoise` and `diff --denoise` (0 = the library's default)."""
    p.add_argument("--search-radius", type=int, default=0, help="search radius A, 1..7 (default 3): offsets up to A samples each way")
    p.add_argument("--patch-radius", type=int, default=0, help="patch radius S, 1..4 (default 2): patches of (2S+1) x (2S+1) samples")
    p.add_argument("--strength", type=float, default=0.0, help="filter strength h in 8-bit code values (default 4.0)")
    p.add_argument("--chroma-strength", type=float, default=0.0, help="strength for the chroma planes (default: --strength)")
    p.add_argument("--temporal-radius", type=int, default=0, metavar="D",
                   help="temporal radius D, 0..3 (default 0): the mean also runs over the search windows of the D frames before and after")
    p.add_argument("--motion-range", type=int, default=0, metavar="PIXELS",
                   help="with --temporal-radius: every 64 x 48 tile gets one vector of up to PIXELS samples each way (even, 0..64) towards "
                        "every neighbour frame and reads the neighbour there; for pans and other motion beyond the search radius (default 0: off)")
    p.add_argument("--joint-chroma", action="store_true",
                   help="luma-guided joint chroma: Cb and Cr share one weight, taken from both and the luma at the same place "
                        "(KNLMeansCL's channels=\"YUV\" in structure; off by default)")
    p.add_argument("--grain-prior", default=None, metavar="TABLE",
                   help="a film grain table (typically a first `diff SOURCE --denoise`) whose luma scaling function the luma strength "
                        "follows: luma is filtered where that grain has one size at every intensity; 8- and 10-bit inputs; off by default")
    p.add_argument("--prior-range", type=int, default=0, metavar="R",
                   help="with --grain-prior: the strongest luma strength over the weakest, 1..16 at 8 bits, 1..4 at 10 (default 4)")
    p.add_argument("--prior-segment", type=int, default=None, metavar="K",
                   help="with --grain-prior: use the table's segment K (from 0) alone instead of the mean of all segments")


    p.add_argument("--auto-prior", action="store_true",
                   help="measure the clip's noise level at each intensity in a pre-pass and let the luma strength follow it: "
                        "--grain-prior without a table (8- and 10-bit inputs; --prior-range applies)")
    p.add_argument("--auto-strength", action="store_true",
                   help="set --strength and --chroma-strength from the noise the pre-pass measures: h = sqrt(2) sigma")
    p.add_argument("--profile-frames", type=int, default=0, metavar="N",
                   help="with --auto-prior / --auto-strength: measure the first N frames only (default 0: all)")
    p.add_argument("--levels-min-count", type=int, default=0, metavar="N",
                   help="with --auto-prior / --auto-strength: smooth samples an intensity bin needs to take part (default 4096)")
    p.add_argument("--auto-temporal", action="store_true",
                   help="with --auto-prior / --auto-strength: measure the noise from the difference of consecutive frames where the "
                        "picture stands still; holds on spatially correlated grain, which the single-frame measurement under-reads; "
                        "motion reads as noise (an upper bound); the pre-pass needs two frames")
    p.add_argument("--chroma-prior", action="store_true",
                   help="with --joint-chroma and --grain-prior or --auto-prior: the chroma strength follows the grain at the luma under "
                        "each sample -- the table's chroma scaling functions, or the chroma noise the pre-pass measured per luma bin; "
                        "--prior-range 1..8 applies; 8-, 10-bit inputs; off by default")
    p.add_argument("--coarse-levels", type=int, default=0, metavar="K",
                   help="coarse levels K, 0..2 (default 0): the 2 x 2 box mean of every frame (K = 2: its box mean as well) goes through the "
                        "same filter and replaces the low frequencies of the result; for grain coarser than a patch, also on a single frame")
    p.add_argument("--coarse-ratio", type=float, default=0.0, metavar="R",
                   help="with --coarse-levels: a level's strengths over those of the level above it, 0.0625..4 (default 1)")


def _denoise_parameters(args) -> dict:
    # (auto_temporal only where it is set: a job without the flag makes the call it made)
    return dict(**(dict(auto_temporal=True) if getattr(args, "auto_temporal", False) else {}), search_radius=args.search_radius, patch_radius=args.patch_radius, strength=args.strength,
                chroma_strength=args.chroma_strength, temporal_radius=args.temporal_radius, joint_chroma=args.joint_chroma,
                grain_prior=args.grain_prior, prior_range=args.prior_range, prior_segment=args.prior_segment, motion_range=args.motion_range,
                auto_prior=args.auto_prior, auto_strength=args.auto_strength, profile_frames=args.profile_frames,
                levels_min_count=args.levels_min_count, chroma_prior=args.chroma_prior, coarse_levels=args.coarse_levels,
                coarse_ratio=args.coarse_ratio)


def _auto_refused(input: str, parameters: dict) -> bool:
    """The refusals of --auto-prior / --auto-strength / --profile-frames / --levels-min-count, each a logged line: True when
    one was logged."""
    import stat

    prior, strength = parameters.get("auto_prior", False), parameters.get("auto_strength", False)
    frames, count = parameters.get("profile_frames", 0), parameters.get("levels_min_count", 0)
    if frames < 0 or count < 0:
        log.error(AUTO_BAD_NUMBER)
        return True
    if parameters.get("auto_temporal", False) and not prior and not strength:
        log.error(AUTO_TEMPORAL_NEEDS_FLAG)
        return True
    if parameters.get("auto_temporal", False) and frames == 1:
        log.error(AUTO_TEMPORAL_NEEDS_TWO)
        return True
    if not prior and not strength:
        if frames or count:
            log.error(AUTO_NEEDS_FLAG)
            return True
        return False
    if prior and parameters.get("grain_prior") is not None:
        log.error(AUTO_PRIOR_AND_TABLE)
        return True
    if strength and (parameters.get("strength", 0.0) or parameters.get("chroma_strength", 0.0)):
        log.error(AUTO_STRENGTH_AND_STRENGTH)
        return True
    try:
        regular = stat.S_ISREG(os.stat(input).st_mode)
    except OSError:
        return False  # (the command says what is wrong with its input)
    if not regular:
        log.error(AUTO_NEEDS_FILE, input)
        return True
    if prior:
        from .ingest import Y4MReader

        try:
            y = Y4MReader(input)
        except ValueError:
            return False
        bit_depth = y.details.bit_depth
        y.close()
        if bit_depth == 12:
            log.error(PRIOR_12_BIT.replace("--grain-prior", "--auto-prior"))
            return True
    return False


def _chroma_prior_refused(parameters: dict) -> bool:
    """The refusals of --chroma-prior, each a logged line: True when one was logged."""
    if not parameters.get("chroma_prior", False):
        return False
    if parameters.get("grain_prior") is None and not parameters.get("auto_prior", False):
        log.error(CHROMA_PRIOR_NEEDS_PRIOR)
        return True
    if not parameters.get("joint_chroma", False):
        log.error(CHROMA_PRIOR_NEEDS_JOINT)
        return True
    if not 0 <= parameters.get("prior_range", 0) <= 8:
        log.error(CHROMA_PRIOR_BAD_RANGE)
        return True
    return False


def _levels_refused(parameters: dict) -> bool:
    """The refusals of --coarse-levels / --coarse-ratio, each a logged line: True when one was logged."""
    k, r = parameters.get("coarse_levels", 0), parameters.get("coarse_ratio", 0.0)
    if not 0 <= k <= 2:
        log.error(BAD_COARSE_LEVELS)
        return True
    if r != 0.0 and not 0.0625 <= r <= 4.0:
        log.error(BAD_COARSE_RATIO)
        return True
    if r != 0.0 and not k:
        log.error(RATIO_NEEDS_LEVELS)
        return True
    return False


def _motion_refused(parameters: dict) -> bool:
    """The refusals of --motion-range, each a logged line: True when one was logged."""
    mr = parameters.get("motion_range", 0)
    if mr % 2 or not 0 <= mr <= 64:
        log.error(BAD_MOTION_RANGE)
        return True
    if mr and not parameters.get("temporal_radius", 0):
        log.error(MOTION_NEEDS_TEMPORAL)
        return True
    return False


def _prior_refused(input: str, outputs, parameters: dict) -> bool:
    """The refusals of --grain-prior / --prior-range / --prior-segment, each a logged line: True when one was logged."""
    from .ingest import Y4MReader
    from .tbl import TblError, parse_tbl_native

    prior, k = parameters.get("grain_prior"), parameters.get("prior_segment")
    if prior is None:
        if parameters.get("prior_range", 0) or k is not None:
            log.error(PRIOR_NEEDS_TABLE)
            return True
        return False
    if any(o is not None and _same_path(prior, o) for o in outputs):
        log.error(SAME_AS_OUTPUT)
        return True
    try:
        with open(prior, "rb") as f:
            segments = parse_tbl_native(f.read())
    except (OSError, TblError) as e:
        log.error(PRIOR_BAD_TABLE, e)
        return True
    if k is not None and not 0 <= k < len(segments):
        log.error(PRIOR_BAD_SEGMENT, k, len(segments))
        return True
    try:
        y = Y4MReader(input)
    except ValueError:
        return False  # (the command says what is wrong with its input)
    bit_depth = y.details.bit_depth
    y.close()
    if bit_depth == 12:
        log.error(PRIOR_12_BIT)
        return True
    return False


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="grav1synth_amd", description="MI355X-native `grav1synth diff`")
    sub = ap.add_subparsers(dest="command", required=True)
    d = sub.add_parser("diff", help="Compares a source video to a denoised video and generates a film grain table (y4m inputs).")
    d.add_argument("source", help="The untouched source file to inspect.")
    d.add_argument("denoised", nargs="?", default=None, help="The denoised file to inspect (or --denoise).")
    d.add_argument("-o", "--output", required=True, help="The path to the output film grain table.")
    d.add_argument("-y", "--overwrite", action="store_true", help="Overwrite the output file without prompting.")
    d.add_argument("-f", "--filters", default=None,
                   help='A semicolon-separated list of filters to apply to the source before running the diff, e.g. '
                        '"crop:top=42,left=64".  crop: top, bottom, left, right.  resize: width, height, alg (hermite, catmullrom, '
                        "mitchell, lanczos, spline36) runs on the device; its arithmetic restates the video-resize crate, which "
                        "is not in the reference tree: the resized planes are UNVERIFIED against grav1synth's (a warning is logged).")
    d.add_argument("--device", type=int, default=-1, help="HIP device ordinal (default: the current device)")
    d.add_argument("--gpus", type=int, default=1,
                   help="shard the frames over the first N devices of the node (one generator each, batches dealt round-robin, "
                        "ordered merge on the host: the same table as one device).  From .y4m files the command is bound by "
                        "reading them (about 25 GB/s, 560 4K 10-bit frames a second) long before a second device matters; "
                        "does not combine with a resize filter or with --device")
    d.add_argument("--devices", default=None, help="the same with an explicit list of HIP ordinals, e.g. 0,2,3")
    d.add_argument("--denoise", action="store_true",
                   help="make the denoised clip on the device (the project's own integer non-local-means filter, see `denoise`) "
                        "instead of reading a DENOISED file; does not combine with --filters, --gpus or --devices")
    d.add_argument("--keep-denoised", default=None, metavar="PATH", help="with --denoise: also write the denoised clip as .y4m")
    _add_denoise_parameters(d)
    e = sub.add_parser("estimate", help="Estimates the amount of noise in a source video, frame by frame (y4m input; the reference's "
                                        "`estimate`, feature \"unstable\").")
    e.add_argument("source", help="The source file to inspect.")
    e.add_argument("-o", "--output", required=True, help="The path to the output file.")
    e.add_argument("-y", "--overwrite", action="store_true", help="Overwrite the output file without prompting.")
    e.add_argument("--device", type=int, default=-1, help="HIP device ordinal (default: the current device)")
    e.add_argument("--levels", metavar="PATH", default=None,
                   help="also write the clip's noise levels: sigma per intensity bin and plane and the strength they imply for "
                        "`denoise`, from the same read of the clip")
    e.add_argument("--levels-temporal", metavar="PATH", default=None,
                   help="also write the clip's temporal noise levels: sigma from the difference of consecutive frames where the "
                        "picture stands still, its ratio to the single-frame sigma (above 1: correlated grain, or motion) and "
                        "the strength it implies, from the same read of the clip")
    e.add_argument("--table", metavar="PATH", default=None,
                   help="also write the clip's own grain table (.tbl): scaling functions from the temporal noise levels, AR "
                        "coefficients from the lagged products of the frame differences where the picture stands still; no "
                        "denoiser is involved")
    e.add_argument("--lags", metavar="PATH", default=None,
                   help="with --table: also write the lag report: per plane the correlation of the frame difference at the "
                        "table's offsets, the coefficients before quantisation and the gain")
    e.add_argument("--table-lag", type=int, default=None, metavar="L", help="with --table: the table's ar_coeff_lag, 1 .. 3 (default 3)")
    e.add_argument("--profile-frames", type=int, default=None, metavar="N", help="with --table: measure the first N frames only (default: all)")
    e.add_argument("--levels-min-count", type=int, default=None, metavar="N",
                   help="with --table: the fewest samples a bin, and pairs a lag, must have (default 4096)")
    r = sub.add_parser("render", help="Synthesizes the film grain of a table onto a video (y4m input and output): what a decoder "
                                      "shows for the clip encoded with the table (AV1 specification, film grain synthesis process).")
    r.add_argument("input", help="The (denoised) file to put grain on.")
    r.add_argument("-g", "--grain", required=True, help="The film grain table.")
    r.add_argument("-o", "--output", required=True, help="The path to the output .y4m.")
    r.add_argument("-y", "--overwrite", action="store_true", help="Overwrite the output file without prompting.")
    r.add_argument("--device", type=int, default=-1, help="HIP device ordinal (default: the current device)")
    r.add_argument("--clip-restricted", action="store_true",
                   help="clip the output to the restricted (studio) range, the sequence's clip_to_restricted_range")
    n = sub.add_parser("denoise", help="Denoises a video (y4m input and output) with the project's own integer-exact non-local-means "
                                       "filter: the structure of ffmpeg's nlmeans / KNLMeansCL, not their output.")
    n.add_argument("input", help="The file to denoise.")
    n.add_argument("-o", "--output", required=True, help="The path to the output .y4m.")
    n.add_argument("-y", "--overwrite", action="store_true", help="Overwrite the output file without prompting.")
    n.add_argument("--device", type=int, default=-1, help="HIP device ordinal (default: the current device)")
    _add_denoise_parameters(n)
    m = sub.add_parser("measure", help="Measures the grain of NOISY against CLEAN (y4m inputs): strength per intensity bin and "
                                       "correlation over the table's lag-3 neighbourhood, exact integers, as a text profile.")
    m.add_argument("noisy", help="The clip with the grain.")
    m.add_argument("clean", help="The clip without it (the intensity the grain is binned by).")
    m.add_argument("-o", "--output", required=True, help="The path to the output profile.")
    m.add_argument("-y", "--overwrite", action="store_true", help="Overwrite the output file without prompting.")
    m.add_argument("--device", type=int, default=-1, help="HIP device ordinal (default: the current device)")
    m.add_argument("--temporal", metavar="PATH", default=None,
                   help="also write the temporal profile: the correlation of the residual with the residual of the frame before")
    m.add_argument("--cross", metavar="PATH", default=None,
                   help="also write the cross-plane profile: the chroma residuals against the luma residual under them and against each other")
    m.add_argument("--scales", metavar="PATH", default=None,
                   help="also write the multi-scale profile: how the residual summed over 2 x 2 .. 32 x 32 boxes grows (grain size)")
    c = sub.add_parser("check", help="Says how well a grain table fits: the profile of SOURCE - DENOISED beside the profile of the "
                                     "table's grain rendered onto DENOISED (y4m inputs).  Reports; passes no verdict.")
    c.add_argument("source", help="The untouched source file.")
    c.add_argument("denoised", help="The denoised file the table was made with.")
    c.add_argument("-g", "--grain", required=True, help="The film grain table.")
    c.add_argument("-o", "--output", required=True, help="The path to the output profile.")
    c.add_argument("-y", "--overwrite", action="store_true", help="Overwrite the output file without prompting.")
    c.add_argument("--device", type=int, default=-1, help="HIP device ordinal (default: the current device)")
    c.add_argument("--clip-restricted", action="store_true",
                   help="render with the output clipped to the restricted (studio) range, as `render --clip-restricted`")
    c.add_argument("--temporal", metavar="PATH", default=None,
                   help="also write the two-column temporal profile: frame-to-frame correlation of both residuals")
    c.add_argument("--cross", metavar="PATH", default=None,
                   help="also write the two-column cross-plane profile: chroma against luma (the table's chroma-from-luma coefficient) "
                        "and Cb against Cr, of both residuals")
    c.add_argument("--scales", metavar="PATH", default=None,
                   help="also write the two-column multi-scale profile: the growth of both residuals over 2 x 2 .. 32 x 32 boxes "
                        "(grain coarser than the table can say, or a denoiser that kept coarse grain)")
    return ap


def diff_denoise_command(source: str, output: str, overwrite: bool = False, device: int = -1, confirm=_confirm,
                         keep_denoised: Optional[str] = None, **parameters) -> int:
    """`diff SOURCE --denoise -o OUT [--keep-denoised PATH]`: the refusals of `diff` for the paths there are, then the loop of
    g1s_diff_y4m_file_denoised.  Returns the number of frames, -1 after a refusal."""
    from .ingest import diff_y4m_file_denoised

    if not 0 <= parameters.get("temporal_radius", 0) <= 3:
        log.error(BAD_TEMPORAL_RADIUS)
        return -1
    if _motion_refused(parameters) or _chroma_prior_refused(parameters) or _levels_refused(parameters):
        return -1
    if _same_path(source, output) or (keep_denoised is not None and (_same_path(source, keep_denoised) or _same_path(keep_denoised, output))):
        log.error(SAME_AS_OUTPUT)
        return -1
    if _prior_refused(source, (output, keep_denoised), parameters) or _auto_refused(source, parameters):
        return -1
    for path in (output, keep_denoised):
        if path is not None and os.path.exists(path) and not overwrite and not confirm(f"File {path} exists. Overwrite?"):
            log.warning(NOT_OVERWRITING)
            return -1
    frames = diff_y4m_file_denoised(source, output, keep_denoised=keep_denoised, device=device, **parameters)
    log.info("Done, wrote output file to %s", output)
    return frames


def diff_command(source: str, denoised: Optional[str], output: str, overwrite: bool = False, filters: Optional[str] = None,
                 device: int = -1, confirm=_confirm, devices: Optional[List[int]] = None, denoise: bool = False,
                 keep_denoised: Optional[str] = None, **parameters) -> int:
    """Returns the number of frame pairs diffed, or -1 when the command refused to run (a logged line, exit 0)."""
    from .filters import FilterChain, FilterError, Resize
    from .ingest import diff_y4m_files

    if denoise or denoised is None or keep_denoised is not None:
        for refused, line in ((denoised is None and not denoise, NO_DENOISED), (denoised is not None and denoise, BOTH_DENOISED),
                              (not denoise, KEEP_NEEDS_DENOISE), (filters is not None, DENOISE_NO_FILTERS),
                              (devices is not None, DENOISE_ONE_DEVICE)):
            if refused:
                log.error(line)
                return -1
        return diff_denoise_command(source, output, overwrite, device, confirm, keep_denoised, **parameters)
    if _same_path(source, output) or _same_path(denoised, output):
        log.error(SAME_AS_OUTPUT)
        return -1
    if _same_path(source, denoised):
        log.error(SAME_INPUTS)
        return -1
    if filters is not None:
        try:
            fc = FilterChain(filters)
        except FilterError as e:
            log.error("Invalid filter chain: %s", e)
            return -1
        resizes = any(isinstance(f, Resize) for f in fc.filters)
        fc.close()
        if resizes and devices is not None and len(devices) > 1:
            log.error("A resize filter does not combine with --gpus / --devices (one chain, one device)")
            return -1
        if resizes and devices is not None:  # (`--devices 2`: one device -- the plain command on it, not the sharded one)
            device, devices = devices[0], None
        if resizes:
            log.warning("resize: the resampling arithmetic restates the video-resize crate (not in the reference tree): the "
                        "resized source, and the table made from it, are UNVERIFIED against grav1synth's")
    if os.path.exists(output) and not overwrite and not confirm(f"File {output} exists. Overwrite?"):
        log.warning(NOT_OVERWRITING)
        return -1
    frames, _unequal = diff_y4m_files(source, denoised, output, device=device, filters=filters, devices=devices)  # (logs "Computed diff for N frames")
    log.info("Done, wrote output file to %s", output)
    return frames


def estimate_command(source: str, output: str, overwrite: bool = False, device: int = -1, confirm=_confirm,
                     levels: Optional[str] = None, levels_temporal: Optional[str] = None, table: Optional[str] = None,
                     table_lag: Optional[int] = None, profile_frames: Optional[int] = None, levels_min_count: Optional[int] = None,
                     lags: Optional[str] = None) -> int:
    """Commands::Estimate (src/main.rs:534-608): the refusals of :541-560, one estimate_plane_noise per frame, "filmgrn1" and a
    "{:.3}" line per frame (-1 for None), "Done, wrote output file to ...".  --levels PATH is a second output, the clip's
    noise levels; --levels-temporal PATH a third, its temporal noise levels; --table PATH the clip's own grain table (with
    --table-lag, --profile-frames, --levels-min-count).  Returns the frame count, -1 after a refusal: a refusal logs its line
    and writes nothing."""
    from .estimate import estimate_y4m_file

    if _same_path(source, output) or any(p is not None and _same_path(source, p) for p in (levels, levels_temporal)):
        log.error(SAME_AS_OUTPUT)
        return -1
    if levels is not None and _same_path(output, levels):
        log.error(SAME_LEVELS)
        return -1
    if levels_temporal is not None and (_same_path(output, levels_temporal) or (levels is not None and _same_path(levels, levels_temporal))):
        log.error(SAME_LEVELS_TEMPORAL)
        return -1
    if table is None and any(v is not None for v in (table_lag, profile_frames, levels_min_count, lags)):
        log.error(TABLE_NEEDS_FLAG)
        return -1
    if table is not None:
        if any(p is not None and _same_path(table, p) for p in (source, output, levels, levels_temporal, lags)) or \
                (lags is not None and any(p is not None and _same_path(lags, p) for p in (source, output, levels, levels_temporal))):
            log.error(SAME_TABLE)
            return -1
        if table_lag is not None and table_lag not in (1, 2, 3):
            log.error(TABLE_BAD_LAG)
            return -1
        if (profile_frames or 0) < 0 or (levels_min_count or 0) < 0:
            log.error(AUTO_BAD_NUMBER)
            return -1
    for path in (output, levels, levels_temporal, table, lags):
        if path is not None and os.path.exists(path) and not overwrite and not confirm(f"File {path} exists. Overwrite?"):
            log.warning(NOT_OVERWRITING)
            return -1
    # (levels_temporal only where it is given: a job without the flag makes the call it made)
    more = {} if levels_temporal is None else dict(levels_temporal=levels_temporal)
    if table is not None:
        from ._lib import G1SError
        from .estimate import TABLE_NEEDS_TWO_FRAMES

        more.update(table=table, table_lag=table_lag or 3, max_frames=profile_frames or 0, min_count=levels_min_count or 0, lags=lags)
        try:
            frames = estimate_y4m_file(source, output, device=device, levels=levels, **more)
        except G1SError as err:
            if TABLE_NEEDS_TWO_FRAMES in str(err):
                log.error(TABLE_NEEDS_TWO)
            else:
                log.error("%s. Exiting.", str(err).split(": ", 1)[-1])
            return -1
    else:
        frames = estimate_y4m_file(source, output, device=device, levels=levels, **more)
    log.info("Done, wrote output file to %s", output)
    if levels is not None:
        log.info("Done, wrote noise levels to %s", levels)
    if levels_temporal is not None:
        log.info("Done, wrote temporal noise levels to %s", levels_temporal)
    if table is not None:
        log.info("Done, wrote the clip's grain table to %s", table)
    if lags is not None:
        log.info("Done, wrote the lag report to %s", lags)
    return frames


def render_command(input: str, table: str, output: str, overwrite: bool = False, device: int = -1, clip_restricted: bool = False,
                   confirm=_confirm) -> int:
    """The refusals of `diff` and `estimate`, then every frame of the input through the table's lookup and the film grain
    synthesis process.  Returns the frame count, -1 after a refusal."""
    from .grain import render_y4m_file

    if _same_path(input, output) or _same_path(table, output):
        log.error(SAME_AS_OUTPUT)
        return -1
    if os.path.exists(output) and not overwrite and not confirm(f"File {output} exists. Overwrite?"):
        log.warning(NOT_OVERWRITING)
        return -1
    frames = render_y4m_file(input, table, output, device=device, clip_to_restricted_range=clip_restricted)
    log.info("Done, wrote output file to %s", output)
    return frames


def denoise_command(input: str, output: str, overwrite: bool = False, device: int = -1, confirm=_confirm, **parameters) -> int:
    """The refusals of the other commands, then every frame of the input through the filter.  Returns the frame count, -1
    after a refusal."""
    from .denoise import denoise_y4m_file

    if not 0 <= parameters.get("temporal_radius", 0) <= 3:
        log.error(BAD_TEMPORAL_RADIUS)
        return -1
    if _motion_refused(parameters) or _chroma_prior_refused(parameters) or _levels_refused(parameters):
        return -1
    if _same_path(input, output):
        log.error(SAME_AS_OUTPUT)
        return -1
    if _prior_refused(input, (output,), parameters) or _auto_refused(input, parameters):
        return -1
    if os.path.exists(output) and not overwrite and not confirm(f"File {output} exists. Overwrite?"):
        log.warning(NOT_OVERWRITING)
        return -1
    frames = denoise_y4m_file(input, output, device=device, **parameters)
    log.info("Done, wrote output file to %s", output)
    return frames


def _temporal_refused(inputs, output: str, temporal: Optional[str]) -> bool:
    """--temporal PATH is an output like -o's: not an input, and not -o's own path."""
    if temporal is None:
        return False
    if any(_same_path(p, temporal) for p in inputs):
        log.error(SAME_AS_OUTPUT)
        return True
    if _same_path(output, temporal):
        log.error(SAME_OUTPUTS)
        return True
    return False


def _cross_refused(inputs, output: str, temporal: Optional[str], cross: Optional[str], clip: str) -> bool:
    """--cross PATH is an output too: not an input, not -o's path, not --temporal's; and the clip needs chroma planes."""
    if cross is None:
        return False
    if any(_same_path(p, cross) for p in inputs):
        log.error(SAME_AS_OUTPUT)
        return True
    if _same_path(output, cross):
        log.error(SAME_CROSS_OUTPUT)
        return True
    if temporal is not None and _same_path(temporal, cross):
        log.error(SAME_CROSS_TEMPORAL)
        return True
    if _y4m_is_monochrome(clip):
        log.error(CROSS_NEEDS_CHROMA)
        return True
    return False


def _scales_refused(inputs, output: str, temporal: Optional[str], cross: Optional[str], scales: Optional[str]) -> bool:
    """--scales PATH is an output too: not an input, not -o's path, not --temporal's, not --cross's."""
    if scales is None:
        return False
    if any(_same_path(p, scales) for p in inputs):
        log.error(SAME_AS_OUTPUT)
        return True
    if _same_path(output, scales):
        log.error(SAME_SCALES_OUTPUT)
        return True
    if temporal is not None and _same_path(temporal, scales):
        log.error(SAME_SCALES_TEMPORAL)
        return True
    if cross is not None and _same_path(cross, scales):
        log.error(SAME_SCALES_CROSS)
        return True
    return False


def _y4m_is_monochrome(path: str) -> bool:
    """Does the .y4m header name a colour space without chroma planes?  (An unreadable file is the reader's to refuse.)"""
    try:
        with open(path, "rb") as f:
            header = f.read(256).split(b"\n", 1)[0]
    except OSError:
        return False
    return header.startswith(b"YUV4MPEG2") and any(t.startswith(b"Cmono") for t in header.split()[1:])


def measure_command(noisy: str, clean: str, output: str, overwrite: bool = False, device: int = -1, confirm=_confirm,
                    temporal: Optional[str] = None, cross: Optional[str] = None, scales: Optional[str] = None) -> int:
    """The refusals of `diff` for two inputs and an output, then the frame pairs until the shorter file ends and the
    profile (with `temporal`, the temporal profile beside it).  Returns the frame count, -1 after a refusal."""
    from .measure import measure_y4m_files

    if _same_path(noisy, output) or _same_path(clean, output):
        log.error(SAME_AS_OUTPUT)
        return -1
    if _same_path(noisy, clean):
        log.error(SAME_INPUTS)
        return -1
    if _temporal_refused((noisy, clean), output, temporal) or _cross_refused((noisy, clean), output, temporal, cross, clean):
        return -1
    if _scales_refused((noisy, clean), output, temporal, cross, scales):
        return -1
    for path in (output, temporal, cross, scales):
        if path is not None and os.path.exists(path) and not overwrite and not confirm(f"File {path} exists. Overwrite?"):
            log.warning(NOT_OVERWRITING)
            return -1
    frames, _unequal = measure_y4m_files(noisy, clean, output, device=device, temporal_output=temporal, cross_output=cross,
                                         scales_output=scales)
    log.info("Done, wrote output file to %s", output)
    if temporal is not None:
        log.info("Done, wrote temporal profile to %s", temporal)
    if cross is not None:
        log.info("Done, wrote cross profile to %s", cross)
    if scales is not None:
        log.info("Done, wrote scale profile to %s", scales)
    return frames


def check_command(source: str, denoised: str, table: str, output: str, overwrite: bool = False, device: int = -1,
                  clip_restricted: bool = False, confirm=_confirm, temporal: Optional[str] = None, cross: Optional[str] = None,
                  scales: Optional[str] = None) -> int:
    """The same refusals (the table is an input too), then the two profiles side by side.  No verdict, no threshold.
    Returns the frame count, -1 after a refusal."""
    from .measure import check_y4m_files

    if _same_path(source, output) or _same_path(denoised, output) or _same_path(table, output):
        log.error(SAME_AS_OUTPUT)
        return -1
    if _same_path(source, denoised):
        log.error(SAME_INPUTS)
        return -1
    if _temporal_refused((source, denoised, table), output, temporal) or _cross_refused((source, denoised, table), output, temporal, cross, denoised):
        return -1
    if _scales_refused((source, denoised, table), output, temporal, cross, scales):
        return -1
    for path in (output, temporal, cross, scales):
        if path is not None and os.path.exists(path) and not overwrite and not confirm(f"File {path} exists. Overwrite?"):
            log.warning(NOT_OVERWRITING)
            return -1
    frames, _unequal = check_y4m_files(source, denoised, table, output, device=device, clip_to_restricted_range=clip_restricted,
                                       temporal_output=temporal, cross_output=cross, scales_output=scales)
    log.info("Done, wrote output file to %s", output)
    if temporal is not None:
        log.info("Done, wrote temporal profile to %s", temporal)
    if cross is not None:
        log.info("Done, wrote cross profile to %s", cross)
    if scales is not None:
        log.info("Done, wrote scale profile to %s", scales)
    return frames


def main(argv: Optional[List[str]] = None) -> int:
    args = build_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(levelname)s %(message)s", stream=sys.stderr)
    if args.command == "diff":
        try:
            devices = None
            if args.gpus < 1:
                raise ValueError("--gpus: at least 1")
            if (args.devices or args.gpus > 1) and args.device >= 0:
                raise ValueError("--device does not combine with --gpus / --devices")
            if args.devices:
                devices = [int(x) for x in args.devices.split(",") if x.strip() != ""]
            elif args.gpus > 1:
                devices = list(range(args.gpus))
            if args.denoise or args.denoised is None or args.keep_denoised is not None:
                diff_command(args.source, args.denoised, args.output, args.overwrite, args.filters, args.device, devices=devices,
                             denoise=args.denoise, keep_denoised=args.keep_denoised, **_denoise_parameters(args))
            else:
                diff_command(args.source, args.denoised, args.output, args.overwrite, args.filters, args.device, devices=devices)
        except Exception as e:  # `?` out of main: the error, a non-zero exit
            log.error("%s", e)
            return 1
    elif args.command == "estimate":
        try:
            estimate_command(args.source, args.output, args.overwrite, args.device, levels=args.levels,
                             **({} if args.levels_temporal is None else dict(levels_temporal=args.levels_temporal)),
                             **({} if all(v is None for v in (args.table, args.table_lag, args.profile_frames, args.levels_min_count, args.lags)) else
                                dict(table=args.table, table_lag=args.table_lag, profile_frames=args.profile_frames, levels_min_count=args.levels_min_count,
                                     lags=args.lags)))
        except Exception as e:
            log.error("%s", e)
            return 1
    elif args.command == "render":
        try:
            render_command(args.input, args.grain, args.output, args.overwrite, args.device, args.clip_restricted)
        except Exception as e:
            log.error("%s", e)
            return 1
    elif args.command == "denoise":
        try:
            denoise_command(args.input, args.output, args.overwrite, args.device, **_denoise_parameters(args))
        except Exception as e:
            log.error("%s", e)
            return 1
    elif args.command == "measure":
        try:
            measure_command(args.noisy, args.clean, args.output, args.overwrite, args.device, temporal=args.temporal, cross=args.cross, scales=args.scales)
        except Exception as e:
            log.error("%s", e)
            return 1
    elif args.command == "check":
        try:
            check_command(args.source, args.denoised, args.grain, args.output, args.overwrite, args.device, args.clip_restricted,
                          temporal=args.temporal, cross=args.cross, scales=args.scales)
        except Exception as e:
            log.error("%s", e)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
