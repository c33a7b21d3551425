"""The device half of the per-frame fold (csrc/latest.hip, G1S_LATEST=device) at the edges of its chunked lists: the strength
pass takes a frame's blocks 1 024 at a time, partitions their terms by bin into lists in LDS and adds every list front to back --
the totals included, as the list of every measured block.  The cases here fill a chunk's lists to the brim (every one of 1 024
blocks measured, and all of them in one bin), leave a short last chunk (tests/test_gpu_latest_wide.py has the chunk edges block by block) and go through the refusals; each compares the device
half's blobs with the host half's, byte for byte.  The last case holds the engine's own choice of the half (G1S_LATEST unset) to
the frame size it is made by."""
from fractions import Fraction

import numpy as np
import pytest

from grav1synth_amd.diff import DiffGenerator, format_tbl
from grav1synth_amd.synth import SynthSpec, make_pair

pytestmark = pytest.mark.gpu


def _blobs(monkeypatch, where, frames, bit_depth=8, lag=3, chroma=True, xdec=1, ydec=1, batch=2):
    monkeypatch.setenv("G1S_LATEST", where)
    g = DiffGenerator(Fraction(24, 1), bit_depth, bit_depth, ar_coeff_lag=lag, luma_only=not chroma, batch_frames=batch, records_only=2)
    for s, d in frames:
        g.diff_frame(s, d, xdec, ydec)
    out = g.take_latest(len(frames) + 8, sync=True).copy()
    g.close()
    return out


def _same(host, dev, n):
    assert host.shape == dev.shape and host.shape[0] == n
    for i in range(n):
        if not np.array_equal(host[i], dev[i]):
            bad = np.flatnonzero(host[i] != dev[i])
            raise AssertionError(f"frame {i}: {bad.size} bytes differ, first at {bad[0]} (of {host.shape[1]})")


def _status(blob):
    return int(np.frombuffer(blob.tobytes()[12:16], np.int32)[0])


def _measured(blob):
    """Blocks that went into the luma strength system (num_equations of plane 0's head, behind the 128-byte header)."""
    return int(np.frombuffer(blob.tobytes()[144:148], np.int32)[0])


def _grey_pair(w, h, seed, level=100, amp=3):
    """A frame pair whose blocks are all flat and all of one intensity bin: grey + a little noise against plain grey."""
    rng = np.random.default_rng(seed)
    shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    src = [(level + rng.integers(-amp, amp + 1, s)).astype(np.uint8) for s in shapes]
    den = [np.full(s, level, np.uint8) for s in shapes]
    return src, den


@pytest.mark.parametrize("spec,lag,chroma", [
    (SynthSpec(1056, 560, 8, textured=False), 3, True),   # 594 blocks, all flat: one short chunk; ragged bottom edge
    (SynthSpec(1504, 1000, 8, textured=False), 2, False), # 1 504 blocks, luma only: a full chunk and a short one; ragged bottom edge
    (SynthSpec(1190, 602, 10, textured=False), 2, True),  # ragged in both directions
    (SynthSpec(1056, 560, 8, textured=False), 3, False),  # luma only
    (SynthSpec(1056, 560, 8), 3, False),                  # luma only, textured: chunks with a few measured blocks
], ids=["all_flat_594", "all_flat_1504_luma_only", "all_flat_ragged", "all_flat_luma_only", "textured_luma_only"])
def test_full_and_short_chunks_give_the_host_halfs_bytes(monkeypatch, spec, lag, chroma):
    frames = [make_pair(spec, k, device="cuda") for k in range(3)]
    host = _blobs(monkeypatch, "host", frames, spec.bit_depth, lag, chroma, spec.xdec, spec.ydec)
    dev = _blobs(monkeypatch, "device", frames, spec.bit_depth, lag, chroma, spec.xdec, spec.ydec)
    _same(host, dev, len(frames))
    assert all(_status(b) == 0 for b in host)
    assert min(_measured(b) for b in host) > (512 if not spec.textured else 1)


def test_every_block_in_one_bin_gives_the_host_halfs_bytes(monkeypatch):
    """1024 x 1120: 1 120 blocks of one mean, nearly all of them flat -- ONE diagonal list and one b list take a whole chunk's
    1 024 terms and a short chunk's, every other list is empty."""
    frames = [_grey_pair(1024, 1120, seed) for seed in (1, 2)]
    host = _blobs(monkeypatch, "host", frames)
    dev = _blobs(monkeypatch, "device", frames)
    _same(host, dev, len(frames))
    assert all(_status(b) == 0 for b in host), [_status(b) for b in host]
    assert all(_measured(b) > 1024 for b in host), [_measured(b) for b in host]


def test_fewer_than_two_flat_blocks_is_the_host_halfs_refusal(monkeypatch):
    """One block in all: "Not enough flat blocks ..." with the host half's status, text and cleared state, next to a good frame
    in the same launch."""
    good = _grey_pair(64, 64, 3)
    one = ([np.full((32, 32), 9, np.uint8), np.full((16, 16), 9, np.uint8), np.full((16, 16), 9, np.uint8)],) * 2
    for frames in ([one], [good, good]):
        host = _blobs(monkeypatch, "host", frames)
        dev = _blobs(monkeypatch, "device", frames)
        _same(host, dev, len(frames))
    assert _status(_blobs(monkeypatch, "device", [one])[0]) == -3


@pytest.mark.parametrize("size,on_device", [((2048, 2048), True), ((2048, 2016), False)], ids=["4096_blocks", "4032_blocks"])
def test_unset_switch_takes_the_device_half_from_4096_blocks(monkeypatch, size, on_device):
    """G1S_LATEST unset: the engine chooses by the frame's size (the device half's solves cost the same for any size, the host half's
    cost goes with the blocks); the table is the explicit host half's either way."""
    spec = SynthSpec(size[0], size[1], 8)
    frames = [make_pair(spec, k, device="cuda") for k in range(2)]
    out = {}
    for where in (None, "host"):
        if where is None:
            monkeypatch.delenv("G1S_LATEST", raising=False)
        else:
            monkeypatch.setenv("G1S_LATEST", where)
        g = DiffGenerator(Fraction(24, 1), 8, 8, batch_frames=2)
        g.set_timing(True)
        for s, d in frames:
            g.diff_frame(s, d, spec.xdec, spec.ydec)
        out[where] = (format_tbl(g.finish()), "k4_latest" in g.kernel_times())
        g.close()
    assert out[None][0] == out["host"][0]
    assert out[None][1] == on_device and not out["host"][1]
