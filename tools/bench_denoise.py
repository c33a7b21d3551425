#!/usr/bin/env python3
"""tools/bench_denoise.py [batches] -- `denoise` on the GPU box: the non-local-means kernel kd_nlm (forms kPlain, kTemporal) over
device-resident frames, 4K 10-bit 4:2:0 and 1080p 8-bit 4:2:0, batches of 64, at the defaults (A = 3, S = 2) and at A = 7, S = 3
with temporal radius 0 and 1, and at the defaults with temporal radius 2; every case without and with joint chroma
(kd_nlm_j in the same form takes the chroma launch's place; "joint_chroma" in the line).  Per case: HIP-event time per batch around the two
launches (timed batches run alone and are waited for), frames a second from it, the kernel's arithmetic as the specification
counts it -- samples x pairs: the unordered pairs A + A (2A + 1) of the frame itself and, per neighbour frame, the (2A + 1)^2
one-sided pairs of rule 6 (a frame at the end of a clip has fewer; the runs are clips of many batches) -- and the job rate
through g1s_denoise_frame with the timing off.  One JSON line per case.  For the kernel trace:
rocprofv3 --kernel-trace --stats -- python tools/bench_denoise.py 1 (a run of its own).

tools/bench_denoise.py [batches] --prior -- the cost of a grain prior (rules 12 - 15): both formats at the defaults with
temporal radius 0 and 1, without and with a curve ("grain_prior" in the line) in one process.  With a curve the timed span
also holds the two kd_curve launches around the luma launch; their own times come from the kernel trace.

tools/bench_denoise.py [batches] --motion-range R[,R...] -- motion for the temporal radius (rules 16 - 20): 4K 10-bit 4:2:0 at
the defaults with temporal radius 1, once for every range R of the list (0: the denoiser without motion, made by the calls
that were there before it).  The timed span holds kd_motion in front of the filter launches; "kd_motion_us_per_frame" is its
own HIP-event time, "filter_us_per_frame" the rest, "motion_candidate_samples" the count that explains the first: per
frame, blocks x neighbours x (R + 1)^2 candidates x up to 768 search-plane samples.

tools/bench_denoise.py [batches] --gain -- the cost of a chroma gain (rules 21 - 24): both formats under joint chroma at
(A 3, S 2, D 0), (A 7, S 3, D 0) and (A 3, S 2, D 1), without and with a gain ("chroma_gain" in the line) in one process, one
denoiser after the other.  The gain is rule 21 at R = 8 on a steep scaling function, so that no entry is the flat gain's and no
path is skipped.  The timed span holds the luma launch, which the gain does not touch, and the joint launch; "luma_only" cases
(the same clip's luma planes alone) give the first, so "joint_launch_us_per_frame" = the span less that.

tools/bench_denoise.py [batches] --levels -- coarse levels (rules 25 - 29): both formats at the defaults with temporal radius 0
and 1, K = 0, 1 and 2 in one process.  "level_us_per_frame" is g1s_denoise_level_time (kd_down, kd_lowres, kd_add and the coarse
levels' own launches, a part of the span), "level_kernels_us_per_frame" the three kernels alone over all levels,
"level_kernel_bytes_per_frame" what they move as the specification counts it (per level with frame bytes N and s samples: kd_down
N + N / 4, kd_lowres N + N / 4 + s / 2, kd_add s / 2 + 2 N) and "level_kernels_GBps" the two together.  "copy_GBps" is a
device-to-device copy of a quarter of a batch's such bytes (half read, half written), four times over, timed with HIP events in the same process."""
import json, os, sys, time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from grav1synth_amd.denoise import Denoiser
from grav1synth_amd.synth import SynthSpec, make_pair

assert torch.cuda.is_available(), "bench_denoise.py needs a GPU"
PRIOR = "--prior" in sys.argv[1:]
GAIN = "--gain" in sys.argv[1:]
LEVELS = "--levels" in sys.argv[1:]
args = [a for a in sys.argv[1:] if a not in ("--prior", "--gain", "--levels")]
MOTION = None
if "--motion-range" in args:
    i = args.index("--motion-range")
    MOTION = [int(r) for r in args[i + 1].split(",")]
    del args[i:i + 2]
batches = int(args[0]) if args else 4
BATCH = 64
if PRIOR:
    from grav1synth_amd.denoise import grain_curve
    from grav1synth_amd.tbl import parse_tbl

    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "reference-example-table.tbl"), "rb") as f:
        PRIOR_SEGMENTS = parse_tbl(f.read())
    CASES = [(3, 2, d, False, c) for d in (0, 1) for c in (False, True)]
elif MOTION is not None:
    CASES = [(3, 2, 1, False, False, r) for r in MOTION]
elif LEVELS:
    # (A, S, D, joint, prior, motion range, what, K)
    CASES = [(3, 2, d, False, False, 0, None, k) for d in (0, 1) for k in (0, 1, 2)]
elif GAIN:
    import numpy as np

    from grav1synth_amd import _lib

    _s = np.where(np.arange(256) < 96, 3, 255).astype(np.uint8)
    STEEP_GAIN = np.zeros(256, np.uint16)
    assert _lib.lib().g1s_denoise_chroma_gain_sigma(_s.ctypes.data, 8, STEEP_GAIN.ctypes.data) == 0 and (STEEP_GAIN != 256).all()
    # (A, S, D, joint, prior, motion range, what: "luma" = the luma planes alone, "joint", "gain")
    CASES = [(a, s, d, True, False, 0, w) for a, s, d in ((3, 2, 0), (7, 3, 0), (3, 2, 1)) for w in ("luma", "joint", "gain")]
else:
    CASES = [(a, s, d, j, False) for a, s, d in ((3, 2, 0), (7, 3, 0), (3, 2, 1), (7, 3, 1), (3, 2, 2)) for j in (False, True)]

FORMATS = (("3840x2160 10-bit 4:2:0", SynthSpec(3840, 2160, 10)), ("1920x1080 8-bit 4:2:0", SynthSpec(1920, 1080, 8)))
for name, spec in FORMATS[:1] if MOTION is not None else FORMATS:
    # 8 distinct noisy frames in, 64 distinct frames out (a batch writes every out plane once)
    ins = [make_pair(spec, k, device="cuda")[0] for k in range(8)]
    outs = [[torch.empty_like(p) for p in ins[0]] for _ in range(BATCH)]
    torch.cuda.synchronize()
    samples = sum(p.numel() for p in ins[0])
    for A, S, D, joint, prior, *rest in CASES:
        kw = dict(curve=grain_curve(PRIOR_SEGMENTS, spec.bit_depth)) if prior else {}
        mr = rest[0] if rest else 0
        if mr:
            kw["motion_range"] = mr
        what = rest[1] if len(rest) > 1 else None
        if what == "gain":
            kw["chroma_gain"] = STEEP_GAIN
        planes = slice(0, 1) if what == "luma" else slice(None)
        K = rest[2] if len(rest) > 2 else 0
        if K:  # (K = 0: the denoiser as the calls before the levels make it)
            kw["coarse_levels"] = K
        dn = Denoiser(spec.bit_depth, batch_frames=BATCH, search_radius=A, patch_radius=S, temporal_radius=D, joint_chroma=joint, **kw)

        def run(nb):
            for k in range(nb * BATCH):
                dn.apply(ins[k % 8][planes], spec.xdec, spec.ydec, sync=False, out=outs[k % BATCH][planes])
            dn.sync()

        run(1)  # warm-up: code objects, buffers
        t0 = time.perf_counter()
        run(batches)
        dt = time.perf_counter() - t0
        dn.kernel_times(True)
        run(batches)
        ms, fr = dn.kernel_times(False)
        ms_motion = dn.motion_time() if mr else 0.0
        level = {}
        if LEVELS:
            ms_level, ms_lk = dn.level_time(), dn.level_kernel_time()
            nbytes = sum(p.numel() * p.element_size() for p in ins[0])
            moved = sum((4.5 * nbytes + samples) / 4 ** l for l in range(K))
            level = {"coarse_levels": K, "level_us_per_frame": ms_level * 1e3 / fr, "level_share_of_span": ms_level / ms, "level_kernels_us_per_frame": ms_lk * 1e3 / fr,
                     "level_kernel_bytes_per_frame": moved}
            if K:
                n = int(moved * BATCH) // 8  # (a copy of n bytes moves 2 n)
                a, b = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                b.copy_(a)
                e0.record()
                for _ in range(4):
                    b.copy_(a)
                e1.record()
                torch.cuda.synchronize()
                level.update({"level_kernels_GBps": moved * fr / (ms_lk * 1e6), "copy_GBps": 8 * n / (e0.elapsed_time(e1) * 1e6)})
                del a, b
        dn.close()
        pairs, temporal_pairs = A + A * (2 * A + 1), 2 * D * (2 * A + 1) ** 2
        print(json.dumps({
            "format": name, "search_radius": A, "patch_radius": S, "temporal_radius": D, "joint_chroma": joint, **({"grain_prior": prior} if PRIOR else {}),
            **({"chroma_gain": what == "gain", "luma_only": what == "luma"} if GAIN else {}), **level, "batch_frames": BATCH, "timed_batches": fr / BATCH,
            "samples_per_frame": samples, "unordered_pairs": pairs, "temporal_pairs": temporal_pairs,
            "kd_nlm_ms_per_batch": ms / (fr / BATCH), "kd_nlm_us_per_frame": ms * 1e3 / fr, "kernel_frames_per_s": fr / (ms * 1e-3),
            "sample_pairs_per_ns": samples * (pairs + temporal_pairs) * fr / (ms * 1e6),
            "job_frames_per_s_untimed": batches * BATCH / dt,
            **({"motion_range": mr, "kd_motion_us_per_frame": ms_motion * 1e3 / fr, "filter_us_per_frame": (ms - ms_motion) * 1e3 / fr,
                "motion_candidate_samples": sum(-(-p.shape[0] // 48) * -(-p.shape[1] // 64) * min(p.shape[0] + 1 >> 1, 24) * min(p.shape[1] + 1 >> 1, 32)
                                                for p in ins[0]) * 2 * D * (mr + 1) ** 2} if MOTION is not None else {}),
        }), flush=True)
