#!/usr/bin/env python3
"""tools/bench_grain.py [batches] -- `render` on the GPU box: film grain synthesis over device-resident frames, 4K 10-bit 4:2:0
and 1080p 8-bit 4:2:0, batches of 64.  Per format: HIP-event time per batch of kg_template and of kg_apply (timed batches run
alone and are waited for), kg_apply's traffic -- every sample read once and written once: 2 x frame bytes -- against the
8 TB/s HBM roofline, and the job rate through g1s_grain_frame with the timing off (batches pipeline on the stream).  One JSON
line per format.  For the kernel trace: rocprofv3 --kernel-trace --stats -- python tools/bench_grain.py 4 (a run of its own)."""
import json, os, sys, time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from grav1synth_amd.diff import GrainTableSegment
from grav1synth_amd.grain import GrainSynthesizer
from grav1synth_amd.synth import SynthSpec, make_pair

assert torch.cuda.is_available(), "bench_grain.py needs a GPU"
batches = int(sys.argv[1]) if len(sys.argv) > 1 else 16
BATCH = 64
seg = GrainTableSegment(
    random_seed=7391, start_time=0, end_time=2 ** 63 - 1,
    scaling_points_y=[(0, 70), (40, 70), (81, 93), (134, 107), (255, 107)], scaling_points_cb=[(0, 99), (255, 99)],
    scaling_points_cr=[(0, 99), (134, 98), (255, 99)], scaling_shift=11, ar_coeff_lag=3,
    ar_coeffs_y=[-1, 8, -12, 15, -5, 2, 2, 7, -19, 37, -40, 18, -3, 1, -10, 33, -65, 86, -20, 5, 1, 11, -30, 76],
    ar_coeffs_cb=[2, 2, -2, 5, 1, -1, 5, 1, -3, 16, -22, 6, 3, -2, 0, 15, -39, 66, -9, 0, 4, 5, -16, 62, 31],
    ar_coeffs_cr=[2, 0, -1, 5, 2, 0, 2, 2, -4, 15, -19, 5, 2, 0, -2, 16, -39, 64, -8, 1, 2, 6, -18, 62, 33],
    ar_coeff_shift=7, cb_mult=128, cb_luma_mult=192, cb_offset=256, cr_mult=128, cr_luma_mult=192, cr_offset=256,
    chroma_scaling_from_luma=False, grain_scale_shift=0, overlap_flag=True)

for name, spec in (("3840x2160 10-bit 4:2:0", SynthSpec(3840, 2160, 10)), ("1920x1080 8-bit 4:2:0", SynthSpec(1920, 1080, 8))):
    # 8 distinct frames in, 64 distinct frames out (a batch writes every out plane once)
    ins = [make_pair(spec, k, device="cuda")[1] for k in range(8)]
    outs = [[torch.empty_like(p) for p in ins[0]] for _ in range(BATCH)]
    torch.cuda.synchronize()
    frame_bytes = sum(p.numel() * p.element_size() for p in ins[0])
    syn = GrainSynthesizer(spec.bit_depth, batch_frames=BATCH)

    def run(nb):
        for k in range(nb * BATCH):
            s = GrainTableSegment(**{**seg.__dict__, "random_seed": (seg.random_seed + 10956 * (k + 1)) & 0xFFFF})
            syn.apply(ins[k % 8], s, spec.xdec, spec.ydec, sync=False, out=outs[k % BATCH])
        syn.sync()

    run(2)  # warm-up: code objects, buffers
    t0 = time.perf_counter()
    run(batches)
    dt = time.perf_counter() - t0
    syn.kernel_times(True)
    run(batches)
    ms_t, ms_a, fr = syn.kernel_times(False)
    syn.close()
    nb = fr / BATCH
    gbs = 2 * frame_bytes * fr / (ms_a * 1e-3) / 1e9
    print(json.dumps({
        "format": name, "batch_frames": BATCH, "timed_batches": nb, "frame_bytes": frame_bytes,
        "kg_template_ms_per_batch": ms_t / nb, "kg_apply_ms_per_batch": ms_a / nb,
        "kg_apply_us_per_frame": ms_a * 1e3 / fr, "kg_apply_GB_s": gbs, "kg_apply_fraction_of_8TB_s": gbs / 8000.0,
        "job_frames_per_s_untimed": batches * BATCH / dt,
    }))
