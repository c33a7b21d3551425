"""The content the lagged noise levels' tests run on (test infrastructure; numpy only): shared by tests/test_nlf_lags_cpu.py,
tests/test_gpu_nlf_lags.py and the sweep, so that no test module imports another."""
from __future__ import annotations

import numpy as np

SUBSAMPLINGS = {"420": (1, 1), "422": (1, 0), "444": (0, 0), "mono": (0, 0)}


def clip_frames(w, h, bd, ss, seed, n=2, amp=2, fade=1, wild=0.03):
    """n frames of one run, [Y] or [Y, U, V] each: a slope per plane, 3 % of its samples wild (edges: with the 20 % of
    tests/test_nlf_t_cpu.py's clip hardly a 2 x 2 box of luma counts), under fresh noise of +- amp eight-bit code values a
    frame, a fade of `fade` such values a frame (up in the left half, down in the right) and from frame 1 on a block that
    changes altogether (what moved)."""
    rng = np.random.default_rng([seed, w, h, bd, 46])
    subx, suby = SUBSAMPLINGS[ss]
    top, up = (1 << bd) - 1, 1 << (bd - 8)
    shapes = [(h, w)] + ([] if ss == "mono" else [((h + suby) >> suby, (w + subx) >> subx)] * 2)
    base = []
    for c, (ph, pw) in enumerate(shapes):
        ys, xs = np.arange(ph)[:, None], np.arange(pw)[None, :]
        p = ((xs * (2 + c) + ys * (3 - c)) * up // 2 + int(rng.integers(top // 8, top // 2))) % (top + 1)
        base.append(np.where(rng.random((ph, pw)) < wild, rng.integers(0, top + 1, (ph, pw)), p))
    frames = []
    for t in range(n):
        planes = []
        for p in base:
            ph, pw = p.shape
            q = p + rng.integers(-amp * up, amp * up + 1, (ph, pw)) + t * fade * up * np.where(np.arange(pw) < pw // 2, 1, -1)[None, :]
            if t:
                y0, x0 = (t * 5) % max(ph - 3, 1), (t * 7) % max(pw - 3, 1)
                q[y0:y0 + max(ph // 4, 2), x0:x0 + max(pw // 4, 2)] += 40 * up
            planes.append(np.clip(q, 0, top).astype(np.uint8 if bd == 8 else np.uint16))
        frames.append(planes)
    return frames


def gpu_content(bd=10, ss="420", w=150, h=75, seed=3, n=3):
    """What tests/test_gpu_nlf_lags.py's format cases run on: odd luma sides over decimated chroma, a fade, noise, a block that
    moved."""
    return clip_frames(w, h, bd, ss, seed=seed, n=n)


def ar_clip(n=3, seed=21, w=96, h=64, bd=10, ss="420"):
    """Frames that stand still under fresh spatially correlated noise (a 3 x 3 box over white noise plus a share of the luma
    noise in chroma), so that every covariance the fit takes is away from zero."""
    rng = np.random.default_rng(seed)
    subx, suby = SUBSAMPLINGS[ss]
    shapes = [(h, w)] + ([] if ss == "mono" else [((h + suby) >> suby, (w + subx) >> subx)] * 2)
    frames = []
    for _ in range(n):
        planes, luma_noise = [], None
        for c, (ph, pw) in enumerate(shapes):
            z = rng.standard_normal((ph + 2, pw + 2 + c))
            g = sum(z[i:i + ph, j:j + pw] for i in range(3) for j in range(3 + c)) * (3.0 + c)
            if c == 0:
                luma_noise = g
            else:
                g = g + 0.5 * luma_noise[::1 + suby, ::1 + subx][:ph, :pw]
            planes.append(np.clip(np.rint(400 + 30 * c + g), 0, 1023).astype(np.uint16))
        frames.append(planes)
    return frames
