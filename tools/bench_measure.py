#!/usr/bin/env python3
"""tools/bench_measure.py [repeats] -- `measure` on the GPU box: km_measure and km_tail over device-resident frame pairs, 4K
10-bit 4:2:0 and 1080p 8-bit 4:2:0, batches of 32, on two contents: the plane-distinct content (tests/content.py) and a clean
frame of one intensity, which puts every sample of a plane into one bin (the worst case for the bin sums).  Per case: HIP-event
time per batch through g1s_measure_set_timing (a warm-up batch, then `repeats` timed batches, each waited for), median and
spread, and the bytes that must be read (both frames once) / time as a fraction of the 8 TB/s roofline.  Beside it, from the
same process, what the project's streaming kernel k_estimate_pk reaches on the same luma plane (its own bytes / its own
time): the yardstick of this box.  One JSON line per case.  For the kernel trace:
rocprofv3 --kernel-trace --stats -- python tools/bench_measure.py 2 (a run of its own).

tools/bench_measure.py --temporal [repeats]: the plain and the temporal meter on the plane-distinct content of both formats,
in one process, in the order plain, temporal, plain, temporal.  A round of a meter is a warm-up batch and `repeats` timed
batches.  Per format one JSON line: km_measure's time a frame (the yardstick; from the plain meter, and beside it from the
temporal meter's own ordinary launches), km_measure_t's time a temporal record, their ratio, and the temporal kernel's bytes
(four planes: both frames of both pairs, once) / time as a fraction of the 8 TB/s roofline.

tools/bench_measure.py --cross [repeats]: a plain, a temporal and a cross meter on the plane-distinct content of both formats, in
one process, in the order plain, temporal, cross, twice.  Per format one JSON line: km_measure_x's time a cross record (the
launch and its summing launch), the plain CHROMA launch (km_measure on Cb and Cr) and km_measure_t's CHROMA launch -- the
yardstick: the cross kernel does 75 lag products a chroma sample against its 50 and reads the full-resolution luma of both
frames in addition -- their ratios, and the cross kernel's bytes (both frames of the pair, once) / time.

tools/bench_measure.py --scales [repeats]: a plain and a scales meter on both formats, in one process, in the order plain,
scales, twice, on the plane-distinct content, on a clean frame of one intensity (one key a round of the bin sums: the best case)
and on a clean luma of random samples (the 2 x 2 boxes of a round spread over many bins: the worst).  Per format and content one
JSON line: km_measure's time a frame from the plain meter (the yardstick) and from the scales meter's own ordinary launches,
km_measure_s's time a scale record (its launches and the summing launch), their ratio, and the scale kernel's bytes (both
frames of the pair once, and for chroma the clean luma once more) / time."""
import json, os, statistics, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from grav1synth_amd.estimate import NoiseEstimator
from grav1synth_amd.measure import GrainMeter
from tests import content as CT

assert torch.cuda.is_available(), "bench_measure.py needs a GPU"
argv = [a for a in sys.argv[1:] if a not in ("--temporal", "--cross", "--scales")]
repeats = int(argv[0]) if argv else 7
BATCH, PEAK = 32, 8e12


def dev(planes):
    return [torch.from_numpy(np.ascontiguousarray(p)).to("cuda") for p in planes]


def temporal_bench():
    for name, (w, h, bd) in (("3840x2160 10-bit 4:2:0", (3840, 2160, 10)), ("1920x1080 8-bit 4:2:0", (1920, 1080, 8))):
        pairs = [CT.make_frames("distinct", w, h, bd, 1, 1, frame=k) for k in range(4)]
        noisy, clean = [dev(s) for s, _d in pairs], [dev(d) for _s, d in pairs]
        torch.cuda.synchronize()
        frame_bytes = sum(p.numel() for p in noisy[0]) * (1 if bd == 8 else 2)
        plain_us, ordinary_us, temporal_us = [], [], []  # a timed batch each: microseconds a frame / a temporal record
        for rounds in range(2):
            for temporal in (False, True):
                m = GrainMeter(bd, batch_frames=BATCH, temporal=temporal)

                def batch():
                    for k in range(BATCH):
                        m.measure(noisy[k % 4], clean[k % 4], 1, 1)
                    m.finish()
                    if temporal:
                        m.finish_temporal()

                batch()  # warm-up: code objects, buffers; the run goes on, so every timed batch has BATCH temporal records
                for _ in range(repeats):
                    a0, n0 = m.kernel_times(True)
                    t0, p0 = m.temporal_kernel_times()
                    batch()
                    a1, n1 = m.kernel_times(False)
                    t1, p1 = m.temporal_kernel_times()
                    (ordinary_us if temporal else plain_us).append((a1 - a0) * 1e3 / (n1 - n0))
                    if temporal:
                        assert p1 - p0 == BATCH
                        temporal_us.append((t1 - t0) * 1e3 / (p1 - p0))
                m.close()
        med = statistics.median
        print(json.dumps({
            "format": name, "content": "distinct", "batch_frames": BATCH, "repeats": repeats, "order": "plain, temporal, plain, temporal",
            "km_measure_us_per_frame_median": med(plain_us), "km_measure_us_min": min(plain_us), "km_measure_us_max": max(plain_us),
            "km_measure_in_temporal_meter_us_per_frame_median": med(ordinary_us),
            "km_measure_t_us_per_record_median": med(temporal_us), "km_measure_t_us_min": min(temporal_us), "km_measure_t_us_max": max(temporal_us),
            "ratio_km_measure_t_over_km_measure": med(temporal_us) / med(plain_us),
            "km_measure_bytes_per_frame": 2 * frame_bytes, "km_measure_fraction_of_8TBps": 2 * frame_bytes / (med(plain_us) * 1e-6) / PEAK,
            "km_measure_t_bytes_per_record": 4 * frame_bytes, "km_measure_t_TBps": 4 * frame_bytes / (med(temporal_us) * 1e-6) / 1e12,
            "km_measure_t_fraction_of_8TBps": 4 * frame_bytes / (med(temporal_us) * 1e-6) / PEAK,
        }), flush=True)


def cross_bench():
    for name, (w, h, bd) in (("3840x2160 10-bit 4:2:0", (3840, 2160, 10)), ("1920x1080 8-bit 4:2:0", (1920, 1080, 8))):
        pairs = [CT.make_frames("distinct", w, h, bd, 1, 1, frame=k) for k in range(4)]
        noisy, clean = [dev(s) for s, _d in pairs], [dev(d) for _s, d in pairs]
        torch.cuda.synchronize()
        frame_bytes = sum(p.numel() for p in noisy[0]) * (1 if bd == 8 else 2)
        us = {"plain_chroma": [], "plain_all": [], "temporal_chroma": [], "temporal_all": [], "cross": [], "plain_chroma_in_cross_meter": []}
        for rounds in range(2):
            for kind in ("plain", "temporal", "cross"):
                m = GrainMeter(bd, batch_frames=BATCH, temporal=kind == "temporal", cross=kind == "cross")

                def batch():
                    for k in range(BATCH):
                        m.measure(noisy[k % 4], clean[k % 4], 1, 1)
                    m.finish()
                    if kind == "temporal":
                        m.finish_temporal()
                    if kind == "cross":
                        m.finish_cross()

                batch()  # warm-up: code objects, buffers; a temporal run goes on, so every timed batch has BATCH temporal records
                for _ in range(repeats):
                    a0, n0 = m.kernel_times(True)
                    t0, p0 = m.temporal_kernel_times()
                    x0, q0 = m.cross_kernel_times()
                    c0, tc0 = m.chroma_kernel_times()
                    batch()
                    a1, n1 = m.kernel_times(False)
                    t1, p1 = m.temporal_kernel_times()
                    x1, q1 = m.cross_kernel_times()
                    c1, tc1 = m.chroma_kernel_times()
                    assert n1 - n0 == BATCH
                    if kind == "plain":
                        us["plain_all"].append((a1 - a0) * 1e3 / BATCH), us["plain_chroma"].append((c1 - c0) * 1e3 / BATCH)
                    elif kind == "temporal":
                        assert p1 - p0 == BATCH
                        us["temporal_all"].append((t1 - t0) * 1e3 / BATCH), us["temporal_chroma"].append((tc1 - tc0) * 1e3 / BATCH)
                    else:
                        assert q1 - q0 == BATCH
                        us["cross"].append((x1 - x0) * 1e3 / BATCH), us["plain_chroma_in_cross_meter"].append((c1 - c0) * 1e3 / BATCH)
                m.close()
        med = statistics.median
        out = {"format": name, "content": "distinct", "batch_frames": BATCH, "repeats": repeats, "order": "plain, temporal, cross, twice"}
        for key, v in us.items():
            out[f"{key}_us_median"], out[f"{key}_us_min"], out[f"{key}_us_max"] = med(v), min(v), max(v)
        out["ratio_km_measure_x_over_km_measure_t_chroma"] = med(us["cross"]) / med(us["temporal_chroma"])
        out["ratio_km_measure_x_over_km_measure_chroma"] = med(us["cross"]) / med(us["plain_chroma"])
        out["km_measure_x_bytes_per_record"] = 2 * frame_bytes
        out["km_measure_x_TBps"] = 2 * frame_bytes / (med(us["cross"]) * 1e-6) / 1e12
        out["km_measure_x_fraction_of_8TBps"] = 2 * frame_bytes / (med(us["cross"]) * 1e-6) / PEAK
        print(json.dumps(out), flush=True)


def scales_bench():
    for name, (w, h, bd) in (("3840x2160 10-bit 4:2:0", (3840, 2160, 10)), ("1920x1080 8-bit 4:2:0", (1920, 1080, 8))):
        pairs = [CT.make_frames("distinct", w, h, bd, 1, 1, frame=k) for k in range(4)]
        for content in ("distinct", "one intensity", "random luma"):
            noisy, clean = [], []
            for k, (src, den) in enumerate(pairs):
                if content != "distinct":  # the same residuals on another clean frame
                    if content == "one intensity":
                        other = [np.full(p.shape, (100 + 20 * c) << (bd - 8), p.dtype) for c, p in enumerate(den)]
                    else:
                        other = [np.random.default_rng([k, c]).integers(0, 1 << bd, p.shape).astype(p.dtype) for c, p in enumerate(den)]
                    src = [np.clip(f.astype(np.int64) + s.astype(np.int64) - d.astype(np.int64), 0, (1 << bd) - 1).astype(d.dtype)
                           for f, s, d in zip(other, src, den)]
                    den = other
                noisy.append(dev(src)), clean.append(dev(den))
            torch.cuda.synchronize()
            bps = 1 if bd == 8 else 2
            frame_bytes = sum(p.numel() for p in noisy[0]) * bps
            luma_bytes = noisy[0][0].numel() * bps
            us = {"plain": [], "plain_in_scales_meter": [], "scales": []}
            for rounds in range(2):
                for scales in (False, True):
                    m = GrainMeter(bd, batch_frames=BATCH, scales=scales)

                    def batch():
                        for k in range(BATCH):
                            m.measure(noisy[k % 4], clean[k % 4], 1, 1)
                        m.finish()
                        if scales:
                            m.finish_scales()

                    batch()  # warm-up: code objects, buffers
                    for _ in range(repeats):
                        a0, n0 = m.kernel_times(True)
                        s0, q0 = m.scales_kernel_times()
                        batch()
                        a1, n1 = m.kernel_times(False)
                        s1, q1 = m.scales_kernel_times()
                        assert n1 - n0 == BATCH
                        us["plain_in_scales_meter" if scales else "plain"].append((a1 - a0) * 1e3 / BATCH)
                        if scales:
                            assert q1 - q0 == BATCH
                            us["scales"].append((s1 - s0) * 1e3 / BATCH)
                    m.close()
            med = statistics.median
            out = {"format": name, "content": content, "batch_frames": BATCH, "repeats": repeats, "order": "plain, scales, twice"}
            for key, v in us.items():
                out[f"{key}_us_median"], out[f"{key}_us_min"], out[f"{key}_us_max"] = med(v), min(v), max(v)
            out["ratio_km_measure_s_over_km_measure"] = med(us["scales"]) / med(us["plain"])
            out["km_measure_s_bytes_per_record"] = 2 * frame_bytes + luma_bytes
            out["km_measure_s_TBps"] = (2 * frame_bytes + luma_bytes) / (med(us["scales"]) * 1e-6) / 1e12
            out["km_measure_s_fraction_of_8TBps"] = (2 * frame_bytes + luma_bytes) / (med(us["scales"]) * 1e-6) / PEAK
            print(json.dumps(out), flush=True)


if "--scales" in sys.argv[1:]:
    scales_bench()
    sys.exit(0)

if "--cross" in sys.argv[1:]:
    cross_bench()
    sys.exit(0)

if "--temporal" in sys.argv[1:]:
    temporal_bench()
    sys.exit(0)


for name, (w, h, bd) in (("3840x2160 10-bit 4:2:0", (3840, 2160, 10)), ("1920x1080 8-bit 4:2:0", (1920, 1080, 8))):
    pairs = [CT.make_frames("distinct", w, h, bd, 1, 1, frame=k) for k in range(4)]
    for content in ("distinct", "one intensity"):
        noisy, clean = [], []
        for src, den in pairs:
            if content == "one intensity":  # the same residuals on a clean frame of one code value a plane
                flat = [np.full(p.shape, (100 + 20 * c) << (bd - 8), p.dtype) for c, p in enumerate(den)]
                src = [np.clip(f.astype(np.int64) + s.astype(np.int64) - d.astype(np.int64), 0, (1 << bd) - 1).astype(d.dtype) for f, s, d in zip(flat, src, den)]
                den = flat
            noisy.append(dev(src)), clean.append(dev(den))
        torch.cuda.synchronize()
        bps = 1 if bd == 8 else 2
        frame_bytes = sum(p.numel() for p in noisy[0]) * bps
        m = GrainMeter(bd, batch_frames=BATCH)

        def batch():
            for k in range(BATCH):
                m.measure(noisy[k % 4], clean[k % 4], 1, 1)
            m.finish()

        batch()  # warm-up: code objects, buffers
        times = []
        for _ in range(repeats):
            a0, _n = m.kernel_times(True)
            batch()
            a1, _n = m.kernel_times(False)
            times.append(a1 - a0)
        m.close()
        # the yardstick: k_estimate_pk over the same luma planes, same batches
        est = NoiseEstimator(bd, batch_frames=BATCH)

        def ebatch():
            for k in range(BATCH):
                est.estimate_frame(noisy[k % 4][0])
            est.finish()

        ebatch()
        etimes = []
        for _ in range(repeats):
            a0, _n = est.kernel_time(True)
            ebatch()
            a1, _n = est.kernel_time(False)
            etimes.append(a1 - a0)
        est.close()
        ms, ems = statistics.median(times), statistics.median(etimes)
        luma_bytes = noisy[0][0].numel() * bps
        print(json.dumps({
            "format": name, "content": content, "batch_frames": BATCH, "repeats": repeats,
            "measure_ms_per_batch_median": ms, "measure_ms_min": min(times), "measure_ms_max": max(times), "measure_us_per_frame": ms * 1e3 / BATCH,
            "bytes_read_per_frame": 2 * frame_bytes, "measure_TBps": 2 * frame_bytes * BATCH / (ms * 1e-3) / 1e12,
            "measure_fraction_of_8TBps": 2 * frame_bytes * BATCH / (ms * 1e-3) / PEAK,
            "estimate_pk_ms_per_batch_median": ems, "estimate_pk_ms_min": min(etimes), "estimate_pk_ms_max": max(etimes),
            "estimate_pk_TBps": luma_bytes * BATCH / (ems * 1e-3) / 1e12, "estimate_pk_fraction_of_8TBps": luma_bytes * BATCH / (ems * 1e-3) / PEAK,
        }), flush=True)
