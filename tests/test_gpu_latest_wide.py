"""k4_latest as a 512-thread workgroup that takes a frame's blocks 1024 at a time (csrc/latest.hip): the chunk edges of that
size -- a frame of exactly one chunk, a last chunk of one block, a last chunk one block short, more than a chunk of blocks in one
bin -- the refusals next to good frames of the same launch, and a job that runs through every slot more than once.  Each case
compares the device half's bytes (blobs, or the table of a whole job) with the host half's."""
from fractions import Fraction

import numpy as np
import pytest

from grav1synth_amd.diff import DiffGenerator, format_tbl
from grav1synth_amd.synth import SynthSpec, make_pair

pytestmark = pytest.mark.gpu


def _blobs(monkeypatch, where, frames, bit_depth=8, batch=2):
    monkeypatch.setenv("G1S_LATEST", where)
    g = DiffGenerator(Fraction(24, 1), bit_depth, bit_depth, batch_frames=batch, records_only=2)
    for s, d in frames:
        g.diff_frame(s, d, 1, 1)
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
    return int(np.frombuffer(blob.tobytes()[144:148], np.int32)[0])  # num_equations of plane 0


def _grey_pair(w, h, seed, level=100, amp=3):
    rng = np.random.default_rng(seed)
    shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    src = [(level + rng.integers(-amp, amp + 1, s)).astype(np.uint8) for s in shapes]
    den = [np.full(s, level, np.uint8) for s in shapes]
    return src, den


@pytest.mark.parametrize("w,h,blocks", [
    (1024, 1024, 1024),  # one chunk to the brim, nothing behind it
    (800, 1312, 1025),   # a last chunk of one block
    (736, 2848, 2047),   # a last chunk one block short
    (1024, 512, 512),    # fewer blocks than one chunk: the second round's threads have nothing
], ids=lambda v: str(v))
def test_chunk_edges_give_the_host_halfs_bytes(monkeypatch, w, h, blocks):
    spec = SynthSpec(w, h, 8, textured=False)
    assert ((w + 31) // 32) * ((h + 31) // 32) == blocks
    frames = [make_pair(spec, k, device="cuda") for k in range(3)]
    host = _blobs(monkeypatch, "host", frames)
    dev = _blobs(monkeypatch, "device", frames)
    _same(host, dev, len(frames))
    assert all(_status(b) == 0 for b in host)
    assert min(_measured(b) for b in host) > blocks // 2  # (all flat: nearly every block is measured)


def test_more_than_a_chunk_in_one_bin_gives_the_host_halfs_bytes(monkeypatch):
    """1024 x 1120: 1120 blocks of one mean -- one diagonal list and one b list take all 1024 terms of the first chunk."""
    frames = [_grey_pair(1024, 1120, seed) for seed in (5, 6)]
    host = _blobs(monkeypatch, "host", frames)
    dev = _blobs(monkeypatch, "device", frames)
    _same(host, dev, len(frames))
    assert all(_status(b) == 0 for b in host), [_status(b) for b in host]
    assert all(_measured(b) > 1024 for b in host), [_measured(b) for b in host]


def test_refused_frames_next_to_good_ones_in_one_launch(monkeypatch):
    """A constant frame (plane 0's AR system is singular) and a frame whose chroma planes carry no noise (their AR systems are
    singular: the chroma fallback, not a refusal) between good frames of the same launch: every blob is the host half's."""
    good = _grey_pair(256, 256, 7)
    constant = ([np.full((256, 256), 7, np.uint8), np.full((128, 128), 7, np.uint8), np.full((128, 128), 7, np.uint8)],) * 2
    quiet_chroma = (good[0], [good[1][0], good[0][1], good[0][2]])
    frames = [good, constant, quiet_chroma, good]
    host = _blobs(monkeypatch, "host", frames, batch=4)
    dev = _blobs(monkeypatch, "device", frames, batch=4)
    _same(host, dev, len(frames))
    assert [_status(b) for b in host] == [0, -4, 0, 0]


def test_a_job_through_every_slot_twice_gives_the_host_halfs_table(monkeypatch):
    """Nine 64-frame launches and a short one -- wide enough for k4_latest to run in its window on the main stream, the next
    batch's finder chain waiting for the batch before (none for the first; in another slot; in a slot used before) -- with a
    sync() in the middle (every queued batch drained) and a second generator behind the first (it borrows the first one's streams
    and events); then the same in 4-frame launches, which keep k4_latest on a stream of its own: the device half's table is the
    host half's."""
    spec = SynthSpec(320, 192, 8)
    pairs = [make_pair(spec, k, device="cuda") for k in range(16)]
    tables = {}
    for where in ("host", "device"):
        monkeypatch.setenv("G1S_LATEST", where)
        out = []
        for job, batch in enumerate((64, 64, 4)):
            g = DiffGenerator(Fraction(24, 1), 8, 8, batch_frames=batch)
            for k in range(batch * 9 + 3):
                s, d = pairs[(k + job) % len(pairs)]
                g.diff_frame(s, d, spec.xdec, spec.ydec)
                if k == batch * 4 + 1:
                    g.sync()  # (a short batch in the middle of the job)
            out.append(format_tbl(g.finish()))
            g.close()
        tables[where] = out
    assert tables["device"] == tables["host"]
