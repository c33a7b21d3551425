"""Motion for the temporal radius without a device: the numpy reference of rules 16 - 20 (tests/denoise_motion_ref.py)
against a plain loop, what the definition promises (an injective key, the zero vector among equals, the pan found), the
property that justifies the feature, and the two refusals of g1s_denoise_new_motion, which need no device."""
from __future__ import annotations

import ctypes as C
import itertools

import numpy as np
import pytest

from tests import denoise_motion_ref as MR
from tests import denoise_ref as R
from tests import denoise_temporal_ref as TR
from tests import motion_content as MC


def _table(bd, S, h):
    from grav1synth_amd.denoise import weight_table

    return weight_table(bd, S, h)


# ----------------------------------------------------------------------------------------- the reference against a loop
def _half_loop(u):
    H, W = u.shape
    out = np.zeros(((H + 1) >> 1, (W + 1) >> 1), np.int64)
    for y in range(out.shape[0]):
        for x in range(out.shape[1]):
            s = sum(int(u[min(2 * y + j, H - 1), min(2 * x + i, W - 1)]) for j in (0, 1) for i in (0, 1))
            out[y, x] = (s + 2) >> 2
    return out


def _search_loop(cur, ref, mr):
    M = mr // 2
    a, b = _half_loop(cur), _half_loop(ref)
    h, w = a.shape
    out = np.zeros((-(-h // 24), -(-w // 32), 2), np.int64)
    for by in range(out.shape[0]):
        for bx in range(out.shape[1]):
            best = None
            for my in range(-M, M + 1):
                for mx in range(-M, M + 1):
                    sad = 0
                    for y in range(by * 24, min(by * 24 + 24, h)):
                        for x in range(bx * 32, min(bx * 32 + 32, w)):
                            sad += abs(int(a[y, x]) - int(b[min(max(y + my, 0), h - 1), min(max(x + mx, 0), w - 1)]))
                    k = MR.key(sad, mx, my, M)
                    if best is None or k < best[0]:
                        best = (k, 2 * mx, 2 * my)
            out[by, bx] = best[1:]
    return out


def _filter_loop(u, v, mv, A, S, tab, q):
    """Rules 1 - 3 of u on its own and rule 19 against v, sample by sample."""
    h, w = u.shape
    cl = lambda p, n: min(max(p, 0), n - 1)  # noqa: E731
    out = np.zeros((h, w), np.int64)
    for y in range(h):
        for x in range(w):
            mx, my = (int(t) for t in mv[y // 48, x // 64])
            num, den = 4096 * int(u[y, x]), 4096
            for nb, ox, oy in ((u, 0, 0), (v, mx, my)):
                for dy in range(-A, A + 1):
                    for dx in range(-A, A + 1):
                        if nb is u and dx == 0 and dy == 0:
                            continue
                        if not (0 <= x + ox + dx < w and 0 <= y + oy + dy < h):
                            continue
                        D = sum((int(u[cl(y + ky, h), cl(x + kx, w)]) - int(nb[cl(y + oy + dy + ky, h), cl(x + ox + dx + kx, w)])) ** 2
                                for ky in range(-S, S + 1) for kx in range(-S, S + 1))
                        wt = int(tab[min(D >> q, 1023)])
                        num += wt * int(nb[y + oy + dy, x + ox + dx])
                        den += wt
            out[y, x] = (num + (den >> 1)) // den
    return out


@pytest.mark.parametrize("w,h", [(1, 1), (2, 2), (5, 3), (7, 8)])
def test_half_is_the_clamped_box_mean(w, h):
    u = np.random.default_rng([w, h]).integers(0, 4096, (h, w))
    assert np.array_equal(MR.half(u), _half_loop(u))


@pytest.mark.parametrize("w,h,mr", [(1, 1, 2), (9, 7, 4), (70, 9, 4), (9, 52, 2)])
def test_search_is_the_plain_loop(w, h, mr):
    rng = np.random.default_rng([w, h, mr])
    cur, ref = rng.integers(0, 256, (h, w)), rng.integers(0, 256, (h, w))
    assert np.array_equal(MR.search(cur, ref, mr), _search_loop(cur, ref, mr))


def test_the_filter_is_the_plain_loop_with_a_vector_a_block():
    rng = np.random.default_rng(5)
    w, h, A, S = 70, 10, 1, 1
    u, v = rng.integers(0, 256, (h, w)), rng.integers(0, 256, (h, w))
    T, q = _table(8, S, 40.0)
    mv = np.array([[[4, -2], [-6, 2]]])
    num, den = MR.sums_plane([u, v], 0, 1, A, S, T, q, 8, vectors={1: mv})
    assert np.array_equal((num + (den >> 1)) // den, _filter_loop(u, v, mv, A, S, T.astype(np.int64), q))


def test_the_key_is_injective_and_prefers_the_zero_vector():
    M = 32
    keys = {MR.key(sad, mx, my, M) for sad in (0, 1, 768 * 4095, 2 * 768 * 4095) for mx in range(-M, M + 1) for my in range(-M, M + 1)}
    assert len(keys) == 4 * (2 * M + 1) ** 2 and max(keys) < 2 ** 63
    assert min((MR.key(7, mx, my, M), mx, my) for mx in range(-M, M + 1) for my in range(-M, M + 1))[1:] == (0, 0)
    assert MR.key(7, M, M, M) < MR.key(8, 0, 0, M), "the SAD decides first"


# ------------------------------------------------------------------------------------------------ what the search finds
@pytest.mark.parametrize("shift", [(10, 0), (-6, 4), (16, -16)])
def test_a_panned_noise_world_gives_exactly_the_pan_in_interior_blocks(shift):
    clean, _ = MC.pan(3, 320, 240, 8, [shift])
    for cur, ref, want in ((clean[0], clean[1], (-shift[0], -shift[1])), (clean[1], clean[0], shift)):
        mv = MR.search(cur, ref, 32)
        assert mv.shape == (5, 5, 2)
        assert (mv[1:-1, 1:-1] == want).all(), mv[1:-1, 1:-1]


def test_a_different_shift_every_interval_is_searched_directly():
    shifts = [(4, 0), (10, 2), (18, -4)]
    clean, _ = MC.pan(4, 256, 192, 8, shifts)
    pos = MC.positions(shifts)
    for t, k in itertools.product(range(4), (-2, -1, 1, 2)):
        if 0 <= t + k < 4:
            want = (pos[t][0] - pos[t + k][0], pos[t][1] - pos[t + k][1])
            assert (MR.search(clean[t], clean[t + k], 64)[1:-1, 1:-1] == want).all(), (t, k)


def test_constant_and_periodic_frames_give_the_zero_vector_everywhere():
    for period in (0, 4):
        a, b = MC.ties(130, 98, 10, 2, period)
        assert not MR.search(a, b, 32).any()


def test_the_two_halves_have_their_own_vectors():
    f = MC.split(6, 256, 96, 8, (8, 2), 2, "x")
    mv = MR.search(f[0], f[1], 32)
    assert (mv[:, :2] == (-8, -2)).all() and (mv[:, 2:] == (8, 2)).all()


# ------------------------------------------------------------------------------------------------------------ the filter
def test_motion_range_zero_is_the_temporal_reference():
    rng = np.random.default_rng(8)
    planes = [rng.integers(0, 1024, (50, 70)).astype(np.uint16) for _ in range(3)]
    T, q = _table(10, 2, 30.0)
    got = MR.denoise_plane_clip(planes, 1, 3, 2, T, q, 0)
    want = TR.denoise_plane_clip(planes, 1, 3, 2, T, q)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_zero_vectors_are_the_temporal_reference():
    rng = np.random.default_rng(9)
    planes = [rng.integers(0, 256, (50, 70)) for _ in range(2)]
    T, q = _table(8, 2, 30.0)
    zero = np.zeros((2, 2, 2), np.int64)
    got = MR.sums_plane(planes, 0, 1, 2, 2, T, q, 8, vectors={1: zero})
    want = TR.sums_plane(planes, 0, 1, 2, 2, T, q)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_on_a_pan_motion_beats_both_the_spatial_and_the_uncompensated_temporal_filter():
    """The property that justifies the feature.  Texture panned 10 samples a frame, 8 bit, Gaussian grain sigma = 3, D = 1,
    A = 3, S = 2, the best h of {1, 1.25, 1.5, 2} sigma for each filter, MSE against the clean frame over the interior."""
    sigma, A, S = 3.0, 3, 2
    clean, noisy = MC.pan(21, 192, 144, 8, [(10, 0), (10, 0)], sigma, "texture")

    def mse(out):
        e = out[16:-16, 16:-16].astype(np.float64) - clean[1][16:-16, 16:-16]
        return float((e * e).mean())

    best = {}
    for f in (1.0, 1.25, 1.5, 2.0):
        T, q = _table(8, S, f * sigma)
        outs = {"spatial": R.denoise_plane(noisy[1], A, S, T, q), "temporal": TR.denoise_plane_clip(noisy, 1, A, S, T, q)[1]}
        num, den = MR.sums_plane(noisy, 1, 1, A, S, T, q, 32)
        outs["motion"] = (num + (den >> 1)) // den
        for k, o in outs.items():
            best[k] = min(best.get(k, 1e9), mse(o))
    print("MSE against clean, best h each:", best)
    assert best["motion"] < best["spatial"] and best["motion"] < best["temporal"], best


# ---------------------------------------------------------------------------------------------------------- the refusals
@pytest.mark.parametrize("mr,D,text", [(3, 1, "motion_range must be even and 0..64"), (66, 1, "motion_range must be even and 0..64"),
                                       (2, 0, "motion_range needs a temporal radius"), (64, 0, "motion_range needs a temporal radius")])
def test_the_refusals_need_no_device(mr, D, text):
    from grav1synth_amd import _lib
    from grav1synth_amd.denoise import denoise_opts

    L = _lib.lib()
    opts = denoise_opts()
    assert not L.g1s_denoise_new_motion(8, C.byref(opts), D, 0, None, None, mr)
    assert L.g1s_last_global_error().decode() == text


@pytest.mark.parametrize("args,text", [(dict(temporal_radius=1, motion_range=3), "--motion-range must be even and 0..64"),
                                       (dict(temporal_radius=1, motion_range=66), "--motion-range must be even and 0..64"),
                                       (dict(temporal_radius=1, motion_range=-2), "--motion-range must be even and 0..64"),
                                       (dict(motion_range=8), "--motion-range moves the neighbour frames")])
def test_the_commands_refuse_with_a_logged_line(tmp_path, caplog, args, text):
    """like BAD_TEMPORAL_RADIUS: a logged line, -1, nothing written, no device looked for"""
    import logging

    from grav1synth_amd.cli import build_parser, denoise_command, diff_command

    src = tmp_path / "s.y4m"
    src.write_bytes(b"YUV4MPEG2 W2 H2 F24:1 Ip C420jpeg\nFRAME\n" + bytes(6))
    with caplog.at_level(logging.ERROR, logger="grav1synth"):
        assert denoise_command(str(src), str(tmp_path / "o.y4m"), **args) == -1
        assert diff_command(str(src), None, str(tmp_path / "o.tbl"), denoise=True, **args) == -1
    assert sum(text in r.getMessage() for r in caplog.records) == 2 and not (tmp_path / "o.y4m").exists() and not (tmp_path / "o.tbl").exists()
    ns = build_parser().parse_args(["denoise", str(src), "-o", "x", "--motion-range", "32", "--temporal-radius", "1"])
    assert ns.motion_range == 32
    assert build_parser().parse_args(["diff", str(src), "--denoise", "-o", "x"]).motion_range == 0
