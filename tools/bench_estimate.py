#!/usr/bin/env python3
"""tools/bench_estimate.py [frames] [--levels] [--levels-temporal] [--lags] -- N4 on the GPU box: `estimate`'s per-frame noise estimator over HBM-resident 4K 10-bit luma
planes: whole-loop rate (FFI call per frame, one launch + one 16-byte D2H per batch of 32) and the kernel alone (HIP events),
against the 8 TB/s HBM roofline (2 bytes per luma pixel: the plane is read once), with the oracle's scalar rate beside it.
--levels: the two launches of the noise level function (k_nlf on luma; on both chroma planes with the luma under them) on the
same 4:2:0 frames in the same process, beside k_estimate: microseconds a frame, the bytes each must read (luma once; luma
again and both chroma planes) and the fraction of the HBM roofline that implies.
--levels-temporal: --levels, and in the same run a temporal meter over the same frames: the two launches of k_nlf_t, which read
each plane of two frames, beside k_nlf's.
--lags: --levels-temporal, and in the same run a lag meter over the same frames: the two launches of k_nlf_lags beside
k_nlf_t's, against the bytes of two frames read once."""
import json, os, sys, time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from grav1synth_amd.estimate import NoiseEstimator
from grav1synth_amd.synth import SynthSpec, make_pair
from tests.oracle_binding import estimate_plane_noise

args = [a for a in sys.argv[1:] if a not in ("--levels", "--levels-temporal", "--lags")]
lags = "--lags" in sys.argv[1:]
levels_temporal = "--levels-temporal" in sys.argv[1:] or lags
levels = "--levels" in sys.argv[1:] or levels_temporal
n = int(args[0]) if args else 2048
spec = SynthSpec(3840, 2160, 10)
frames = [make_pair(spec, k, device="cuda")[0] for k in range(64)]
planes = [f[0] for f in frames]
torch.cuda.synchronize()
out = {}
for rep in range(3):
    est = NoiseEstimator(10, batch_frames=32)
    est.kernel_time(True)
    t0 = time.perf_counter()
    for k in range(n):
        est.estimate_frame(planes[k % 64])
    got = est.finish()
    dt = time.perf_counter() - t0
    ms, fr = est.kernel_time(True)
    est.close()
px = spec.width * spec.height
out["frames"] = n
out["loop_Mpx_s"] = n * px / dt / 1e6
out["kernel_us_per_frame"] = ms * 1e3 / fr
out["kernel_GB_s"] = 2 * px * fr / (ms * 1e-3) / 1e9
out["kernel_roofline_frac"] = out["kernel_GB_s"] / 8000.0
p0 = planes[0].cpu().numpy()
t0 = time.perf_counter()
want = estimate_plane_noise(p0, 10)
out["oracle_Mpx_s_one_thread"] = px / (time.perf_counter() - t0) / 1e6
assert got[0] == want, (got[0], want)
out["estimate_frame0"] = got[0]
if levels:
    from grav1synth_amd.estimate import NoiseLevelMeter

    for rep in range(3):
        meter = NoiseLevelMeter(10, batch_frames=32)
        meter.kernel_times(True)
        for k in range(n):
            meter.frame(frames[k % 64], spec.xdec, spec.ydec)
            if (k + 1) % 256 == 0 or k + 1 == n:
                recs = meter.finish()  # (the last call's records are looked at below)
        ms_l, ms_c, fr = meter.kernel_times(True)
        meter.close()
    cpx = sum(int(p.numel()) for p in frames[0][1:])
    luma_bytes, chroma_bytes = 2 * px, 2 * px + 2 * cpx
    out["levels_luma_us_per_frame"] = ms_l * 1e3 / fr
    out["levels_chroma_us_per_frame"] = ms_c * 1e3 / fr
    out["levels_luma_bytes"], out["levels_chroma_bytes"] = luma_bytes, chroma_bytes
    out["levels_luma_roofline_frac"] = luma_bytes * fr / (ms_l * 1e-3) / 1e9 / 8000.0
    out["levels_chroma_roofline_frac"] = chroma_bytes * fr / (ms_c * 1e-3) / 1e9 / 8000.0
    out["levels_luma_over_estimate"] = out["levels_luma_us_per_frame"] / out["kernel_us_per_frame"]
    n0, a0 = int(recs[-1]["n"][0].sum()), int(recs[-1]["a"][0].sum())
    k_last = (n - 1) % 64
    assert float(a0) / float(6 * n0) * 1.2533141373155003 == got[k_last], "the luma totals are the estimator's sums"
if levels_temporal:
    for rep in range(3):
        meter = NoiseLevelMeter(10, batch_frames=32, temporal=True)
        meter.kernel_times(True)
        for k in range(n):
            meter.frame(frames[k % 64], spec.xdec, spec.ydec)
            if (k + 1) % 256 == 0 or k + 1 == n:
                recs_t, trecs = meter.finish(), meter.finish_temporal()
        ms_tl, ms_tc, pairs = meter.kernel_times_temporal()
        ms_l2, ms_c2, fr2 = meter.kernel_times(True)
        meter.close()
    assert pairs == n - 1 and recs_t[-1].tobytes() == recs[-1].tobytes(), "the ordinary records are a plain meter's"
    out["levels_t_pairs"] = pairs
    out["levels_t_luma_us_per_pair"] = ms_tl * 1e3 / pairs
    out["levels_t_chroma_us_per_pair"] = ms_tc * 1e3 / pairs
    out["levels_t_luma_bytes"], out["levels_t_chroma_bytes"] = 2 * luma_bytes, 2 * chroma_bytes
    out["levels_t_luma_roofline_frac"] = 2 * luma_bytes * pairs / (ms_tl * 1e-3) / 1e9 / 8000.0
    out["levels_t_chroma_roofline_frac"] = 2 * chroma_bytes * pairs / (ms_tc * 1e-3) / 1e9 / 8000.0
    out["levels_t_luma_over_levels"] = out["levels_t_luma_us_per_pair"] / out["levels_luma_us_per_frame"]
    out["levels_t_chroma_over_levels"] = out["levels_t_chroma_us_per_pair"] / out["levels_chroma_us_per_frame"]
    out["levels_luma_us_per_frame_in_the_temporal_meter"] = ms_l2 * 1e3 / fr2
    out["levels_t_counting_luma_last_pair"] = int(trecs[-1]["n"][0].sum())
if lags:
    for rep in range(3):
        meter = NoiseLevelMeter(10, batch_frames=32, lags=True)
        meter.kernel_times(True)
        for k in range(n):
            meter.frame(frames[k % 64], spec.xdec, spec.ydec)
            if (k + 1) % 256 == 0 or k + 1 == n:
                recs_l, trecs_l, lrecs = meter.finish(), meter.finish_temporal(), meter.finish_lags()
        ms_ll, ms_lc, lpairs = meter.kernel_times_lags()
        ms_tl2, ms_tc2, pairs2 = meter.kernel_times_temporal()
        meter.close()
    assert lpairs == n - 1 and trecs_l[-1].tobytes() == trecs[-1].tobytes(), "the temporal records are a temporal meter's"
    assert int(lrecs[-1]["n"][0, 0]) == int(trecs[-1]["n"][0].sum()) and int(lrecs[-1]["r"][0, 0]) == int(trecs[-1]["q"][0].sum())
    out["lags_pairs"] = lpairs
    out["lags_luma_us_per_pair"] = ms_ll * 1e3 / lpairs
    out["lags_chroma_us_per_pair"] = ms_lc * 1e3 / lpairs
    out["lags_luma_roofline_frac"] = 2 * luma_bytes * lpairs / (ms_ll * 1e-3) / 1e9 / 8000.0
    out["lags_chroma_roofline_frac"] = 2 * chroma_bytes * lpairs / (ms_lc * 1e-3) / 1e9 / 8000.0
    out["lags_luma_over_levels_t"] = out["lags_luma_us_per_pair"] / out["levels_t_luma_us_per_pair"]
    out["lags_chroma_over_levels_t"] = out["lags_chroma_us_per_pair"] / out["levels_t_chroma_us_per_pair"]
    out["levels_t_luma_us_per_pair_in_the_lag_meter"] = ms_tl2 * 1e3 / pairs2
print(json.dumps(out))
