#!/usr/bin/env python3
"""tools/bench_surface.py [repeats] -- the surface converter on the GPU box: ks_unpack and ks_pack over device-resident frames,
3840x2160 P010 4:2:0 and 1920x1080 NV12, batches of 32 distinct frames.  Per format and direction: HIP-event time per batch
through g1s_surface_set_timing (a warm-up batch, then `repeats` timed batches, each waited for), median, min and max, and the
bytes read + written / time.  The yardstick, from the same process: hipMemcpy2DAsync, device to device, of the same planes'
bytes (every plane of the 32 surfaces into a plane of its own shape) on a non-blocking stream with HIP events round the 32
frames' copies, timed the same way: what this box's own copy reaches on exactly the bytes the kernels must move.  (The
converter's stream is inside the library; the yardstick's is another of the same kind.)  One JSON line per case.
G1S_LIB=.../libg1s_v_NAME.so runs a variant build (make variant), e.g. the non-temporal one.  For the kernel trace:
rocprofv3 --kernel-trace --stats -- python tools/bench_surface.py 2 (a run of its own)."""
import ctypes as C
import json, os, statistics, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from grav1synth_amd import _lib
from grav1synth_amd.surface import Surface, SurfaceConverter

assert torch.cuda.is_available(), "bench_surface.py needs a GPU"
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 7
BATCH = 32

_lib.lib()
# the HIP runtime of this process (the one torch brought), by the path it is mapped from
hip_path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
hip = C.CDLL(hip_path)
hip.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
hip.hipStreamSynchronize.argtypes = [C.c_void_p]
D2D, NON_BLOCKING = 3, 1


def ok(rc):
    assert rc == 0, f"HIP error {rc}"


stream, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
ok(hip.hipStreamCreateWithFlags(C.byref(stream), NON_BLOCKING))
ok(hip.hipEventCreate(C.byref(ev0)))
ok(hip.hipEventCreate(C.byref(ev1)))


def rand(shape, dtype, top):
    return torch.randint(0, top + 1, shape, dtype=torch.int32, device="cuda").to(dtype)


def spread(times):
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times)}


for name, (w, h, bd) in (("3840x2160 P010 4:2:0", (3840, 2160, 10)), ("1920x1080 NV12", (1920, 1080, 8))):
    dt = torch.uint8 if bd == 8 else torch.uint16
    bps = 1 if bd == 8 else 2
    ch, cw = (h + 1) >> 1, (w + 1) >> 1
    surfaces = [[rand((h, w), dt, 255 if bd == 8 else 65535), rand((ch, 2 * cw), dt, 255 if bd == 8 else 65535)] for _ in range(BATCH)]
    frames = [[rand((h, w), dt, (1 << bd) - 1), rand((ch, cw), dt, (1 << bd) - 1), rand((ch, cw), dt, (1 << bd) - 1)] for _ in range(BATCH)]
    surfaces_out = [[torch.empty_like(p) for p in s] for s in surfaces]
    frames_out = [[torch.empty_like(p) for p in f] for f in frames]
    torch.cuda.synchronize()
    frame_bytes = sum(p.numel() for p in surfaces[0]) * bps
    conv = SurfaceConverter(bd, batch_frames=BATCH)

    def unpack_batch():
        for k in range(BATCH):
            conv.unpack(Surface(surfaces[k], bd), out=frames_out[k], sync=False)
        conv.sync()

    def pack_batch():
        for k in range(BATCH):
            conv.pack(frames[k], out=surfaces_out[k], sync=False)
        conv.sync()

    def copy_batch():
        ok(hip.hipEventRecord(ev0, stream))
        for k in range(BATCH):
            for src, dst in zip(surfaces[k], surfaces_out[k]):
                row = src.shape[1] * bps
                ok(hip.hipMemcpy2DAsync(dst.data_ptr(), row, src.data_ptr(), row, row, src.shape[0], D2D, stream))
        ok(hip.hipEventRecord(ev1, stream))
        ok(hip.hipStreamSynchronize(stream))
        ms = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1))
        return ms.value

    results = {}
    for what, batch in (("unpack", unpack_batch), ("pack", pack_batch)):
        batch()  # warm-up: code objects, buffers
        times = []
        for _ in range(repeats):
            a0, _n = conv.kernel_time(True)
            batch()
            a1, _n = conv.kernel_time(False)
            times.append(a1 - a0)
        results[what] = times
    conv.close()
    copy_batch()
    copies = [copy_batch() for _ in range(repeats)]
    for what in ("unpack", "pack"):
        t, c = spread(results[what]), spread(copies)
        print(json.dumps({
            "format": name, "direction": what, "batch_frames": BATCH, "repeats": repeats, "lib": os.path.basename(_lib.LIB_PATH),
            "kernel": t, "kernel_us_per_frame": t["median_ms"] * 1e3 / BATCH, "bytes_read_plus_written_per_frame": 2 * frame_bytes,
            "kernel_TBps": 2 * frame_bytes * BATCH / (t["median_ms"] * 1e-3) / 1e12,
            "memcpy2d": c, "memcpy2d_TBps": 2 * frame_bytes * BATCH / (c["median_ms"] * 1e-3) / 1e12,
            "kernel_over_memcpy2d": t["median_ms"] / c["median_ms"], "target": 1.15,
        }), flush=True)
    del surfaces, frames, surfaces_out, frames_out
    torch.cuda.empty_cache()
