"""`denoise`: the project's integer-exact non-local-means filter on an MI355X -- the clip `diff` compares the source with.

HIP kernels behind g1s_denoise_* (include/g1s_diff.h, where the filter is defined); no CPU fallback.  This is the
project's own definition of non-local means: the structure of ffmpeg's nlmeans and of KNLMeansCL, not their bits.

>>> dn = Denoiser(10, strength=4.0)
>>> clean = dn.apply([y, u, v])                 # torch device tensors stay on the device; numpy in, numpy out
>>> clips = Denoiser(10, temporal_radius=2).denoise_clip(frames)   # the mean also runs over 2 frames either side
>>> denoise_y4m_file("grainy.y4m", "clean.y4m", temporal_radius=1)
>>> Denoiser(10, joint_chroma=True).apply([y, u, v])   # Cb and Cr share one weight, guided by the luma at the same place
>>> Denoiser(10, curve=grain_curve(segments, 10)).apply([y, u, v])   # luma strength follows a grain table's scaling function
>>> denoise_y4m_file("grainy.y4m", "clean.y4m", grain_prior="first_pass.tbl")
>>> Denoiser(10, temporal_radius=1, motion_range=32).denoise_clip(frames)   # a pan: each tile reads its neighbours where it finds them
>>> Denoiser(10, joint_chroma=True, chroma_gain=chroma_gain(segments)).apply([y, u, v])   # chroma strength follows the grain at the luma under it
>>> denoise_y4m_file("grainy.y4m", "clean.y4m", grain_prior="first_pass.tbl", joint_chroma=True, chroma_prior=True)
>>> Denoiser(10, coarse_levels=2).apply([y, u, v])   # coarse grain: the 2 x 2 and 4 x 4 box means are filtered as well
"""
from __future__ import annotations

import ctypes as C
import logging
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import G1SDenoiseOpts, G1SError
from ._frame_op import FrameOp

log = logging.getLogger("grav1synth")


def denoise_opts(device: int = -1, batch_frames: int = 0, search_radius: int = 0, patch_radius: int = 0, strength: float = 0.0,
                 chroma_strength: float = 0.0) -> G1SDenoiseOpts:
    """g1s_denoise_opts_t; a zero field means its default (A = 3, S = 2, h = 4.0, chroma = luma)."""
    o = G1SDenoiseOpts()
    o.struct_size = C.sizeof(G1SDenoiseOpts)
    o.device = device
    o.batch_frames = batch_frames
    o.search_radius = search_radius
    o.patch_radius = patch_radius
    o.strength = strength
    o.chroma_strength = chroma_strength
    return o


def _flags(joint_chroma: bool) -> int:
    return _lib.G1S_DENOISE_JOINT_CHROMA if joint_chroma else 0


def weight_table(bit_depth: int, patch_radius: int = 2, strength: float = 4.0, joint_chroma: bool = False) -> Tuple[np.ndarray, int]:
    """(T, q): the 1024 uint16 weights and the shift the kernels use for these parameters (host only, no device needed).
    joint_chroma: the table of the joint chroma filter (rule 10; `strength` is the chroma strength)."""
    L = _lib.lib()
    t = np.zeros(1024, np.uint16)
    q = C.c_uint32()
    rc = L.g1s_denoise_weights_ex(bit_depth, patch_radius, float(strength), _flags(joint_chroma), t.ctypes.data, C.byref(q))
    if rc:
        raise G1SError(rc, L.g1s_last_global_error().decode())
    return t, int(q.value)


def grain_curve(segments: Sequence, bit_depth: int, range: int = 0, segment: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(fwd, inv): the variance-stabilising curve of a grain table's luma scaling function and its inverse (rules 12 and 13
    of include/g1s_diff.h; host only, no device needed).  segments: GrainTableSegment objects; the curve is made from
    their unweighted mean, or from segments[segment] alone.  range R: the strongest strength over the weakest, 1 ..
    2^(12 - bit_depth), 0 = min(4, that).  fwd has 1 << bit_depth uint16 entries, inv 4096."""
    L = _lib.lib()
    segments = list(segments)
    if segment is not None:
        if not 0 <= segment < len(segments):
            raise G1SError(-1, f"grain prior: segment {segment} is not in the table ({len(segments)} segments)")
        segments = [segments[segment]]
    arr = (_lib.G1SSegment * max(len(segments), 1))(*[s.to_c() for s in segments])
    fwd = np.zeros(1 << bit_depth if 0 < bit_depth <= 12 else 1, np.uint16)
    inv = np.zeros(4096, np.uint16)
    rc = L.g1s_denoise_curve(arr, len(segments), bit_depth, range & 0xFFFFFFFF, fwd.ctypes.data, inv.ctypes.data)
    if rc:
        raise G1SError(rc, L.g1s_last_global_error().decode())
    return fwd, inv


def chroma_gain(segments: Sequence, range: int = 0, segment: Optional[int] = None) -> np.ndarray:
    """m[256]: the chroma gain of a grain table's chroma scaling functions at the luma under them (rules 22 and 21 of
    include/g1s_diff.h; host only, no device needed), as Denoiser(chroma_gain=...) takes it.  segments: GrainTableSegment
    objects; the gain is made from the unweighted mean of both chroma planes of all of them, or of segments[segment] alone.
    range R: the strongest strength over the weakest, 1 .. 8, 0 = 4.  256 uint16 entries, a Q8 multiplier of the distance:
    256 where the grain has its mean size."""
    L = _lib.lib()
    segments = list(segments)
    if segment is not None:
        if not 0 <= segment < len(segments):
            raise G1SError(-1, f"grain prior: segment {segment} is not in the table ({len(segments)} segments)")
        segments = [segments[segment]]
    arr = (_lib.G1SSegment * max(len(segments), 1))(*[s.to_c() for s in segments])
    gain = np.zeros(256, np.uint16)
    rc = L.g1s_denoise_chroma_gain(arr, len(segments), range & 0xFFFFFFFF, gain.ctypes.data)
    if rc:
        raise G1SError(rc, L.g1s_last_global_error().decode())
    return gain


class Denoiser(FrameOp):
    _name = "denoise"

    def __init__(self, bit_depth: int, *, device: int = -1, batch_frames: int = 0, search_radius: int = 0, patch_radius: int = 0,
                 strength: float = 0.0, chroma_strength: float = 0.0, temporal_radius: int = 0, joint_chroma: bool = False,
                 curve: Optional[Tuple[np.ndarray, np.ndarray]] = None, motion_range: int = 0, chroma_gain: Optional[np.ndarray] = None,
                 coarse_levels: int = 0, coarse_ratio: float = 0.0):
        """temporal_radius D (0..3): the frames handed over between two sync() calls are a clip, and a frame's mean also
        runs over the D frames before and the D frames after it that the clip has.  joint_chroma: the two chroma planes
        share one weight, taken from Cb, Cr and the input luma at chroma resolution (rules 8 - 11 of include/g1s_diff.h);
        luma, and a luma-only frame, are filtered as without it.  curve = (fwd, inv) of grain_curve(): luma is filtered in
        the domain where the prior's grain has one size at every intensity (rules 12 - 15); chroma as without it.
        motion_range Mr (even, 0..64, needs a temporal radius): every 64 x 48 tile gets one vector of up to Mr samples each
        way towards every neighbour frame, found by a coarse search on the device, and reads the neighbour there (rules
        16 - 20); 0 is the filter without it.  chroma_gain: m[256] of chroma_gain() or estimate.noise_chroma_prior(), or any
        256 values in 1 .. 16384 (needs joint_chroma): the weight of a chroma pair is taken at its distance times the mean of
        m at the guide under its two ends, over 256 (rules 21 - 24); luma never sees it.  coarse_levels K (0..2): the 2 x 2 box mean
        of every frame goes through the same filter (K = 2: its box mean as well) and replaces the low frequencies of the
        result, for grain coarser than a patch (rules 25 - 29); coarse_ratio: a level's strengths over those of the level above
        it, 0.0625 .. 4, 0 = 1.  K = 0 is the filter without it."""
        self._L = _lib.lib()
        self.bit_depth = bit_depth
        self.temporal_radius = temporal_radius
        self.joint_chroma = bool(joint_chroma)
        self.motion_range = motion_range
        opts = denoise_opts(device, batch_frames, search_radius, patch_radius, strength, chroma_strength)
        gain = fwd = inv = None  # a feature that is off: a null pointer to the last rung of g1s_denoise_new*
        if chroma_gain is not None:
            gain = np.ascontiguousarray(chroma_gain, np.uint16)
            if gain.shape != (256,) or not np.array_equal(gain, np.asarray(chroma_gain)):
                raise G1SError(-1, "chroma gain: 256 entries in 1..16384")
        if curve is not None:
            fwd, inv = (np.ascontiguousarray(a, np.uint16) for a in curve)
            if bit_depth in (8, 10) and (fwd.shape != (1 << bit_depth,) or inv.shape != (4096,)):
                raise G1SError(-1, f"curve: fwd must have {1 << bit_depth} entries and inv 4096")
        self.coarse_levels = coarse_levels
        self._h = self._L.g1s_denoise_new_levels(bit_depth, C.byref(opts), temporal_radius & 0xFFFFFFFF, _flags(joint_chroma),
                                                 None if fwd is None else fwd.ctypes.data, None if inv is None else inv.ctypes.data,
                                                 motion_range & 0xFFFFFFFF, None if gain is None else gain.ctypes.data,
                                                 coarse_levels & 0xFFFFFFFF, float(coarse_ratio))
        if not self._h:
            raise G1SError(-1, self._L.g1s_last_global_error().decode())
        self._keep: list = []  # (frame number, planes): what the queued kernels and the frames to come still read or write
        self._frames = 0       # handed over since the denoiser was made, as g1s_denoise_drain counts

    def apply(self, frame_planes: Sequence, xdec: int = 1, ydec: int = 1, *, sync: bool = True, out: Optional[Sequence] = None) -> List:
        """One frame through the filter: new planes of the same kind -- torch device tensors stay on the device, host planes
        go through host frames.  sync = False queues the frame (a batch goes out as one launch per plane class): the
        returned planes are complete after sync(), or once drain() has counted the frame.  sync = True ends the clip with
        this frame: with a temporal radius it is a one-frame clip unless frames were queued before it (denoise_clip takes
        a whole clip)."""
        planes, out, keep, fin, fout = self._frame_pair(frame_planes, xdec, ydec, out)
        self._keep.append((self._frames, (keep, planes, out)))
        self._check(self._L.g1s_denoise_frame(self._h, C.byref(fin), C.byref(fout)))
        self._frames += 1
        if sync:
            self.sync()
        return out

    def denoise_clip(self, frames: Sequence[Sequence], xdec: int = 1, ydec: int = 1) -> List[List]:
        """The frames of one clip through the filter, in order: queued, then sync().  Returns the output frames."""
        outs = [self.apply(f, xdec, ydec, sync=False) for f in frames]
        self.sync()
        return outs

    def drain(self) -> int:
        """Launches every queued frame whose later neighbours are there and waits; the clip goes on.  Returns how many frames
        since the denoiser was made are complete (with temporal radius D the last D frames wait for sync() or more frames)."""
        n = C.c_uint64()
        self._check(self._L.g1s_denoise_drain(self._h, C.byref(n)))
        # frame k's input is a neighbour of the frames up to k + D
        self._keep = [e for e in self._keep if e[0] + self.temporal_radius >= n.value]
        return int(n.value)

    def sync(self) -> None:
        """Launches what is queued and waits.  The clip ends here."""
        self._check(self._L.g1s_denoise_sync(self._h))
        self._keep.clear()

    def motion_vectors(self, cur: Sequence, ref: Sequence, xdec: int = 1, ydec: int = 1) -> List[np.ndarray]:
        """Stage 1 alone: the vectors of frame `cur` towards frame `ref` (rules 16 - 18 and 20), one int16 array of shape
        (block rows, block columns, 2) a plane, (mx, my) in full-resolution samples of that plane.  Under joint_chroma the two
        chroma planes carry the same shared vectors.  Does not touch a clip in progress."""
        a, b, keep, fa, fb = self._frame_pair(cur, xdec, ydec, list(ref))
        shapes = [(-(-p.shape[0] // 48), -(-p.shape[1] // 64)) for p in a]
        mv = [np.zeros(s + (2,), np.int16) for s in shapes]
        ptrs = (C.c_void_p * 3)(*[m.ctypes.data for m in mv])
        caps = (C.c_size_t * 3)(*[s[0] * s[1] for s in shapes])
        self._check(self._L.g1s_denoise_motion_search(self._h, C.byref(fa), C.byref(fb), ptrs, caps))
        del keep
        return mv

    def motion_time(self) -> float:
        """ms in kd_motion of the timed batches so far (a part of kernel_times()' first value)."""
        a = C.c_double()
        self._L.g1s_denoise_motion_time(self._h, C.byref(a))
        return a.value

    def level_time(self) -> float:
        """ms in kd_down, kd_lowres, kd_add and the coarse levels of the timed batches so far (a part of kernel_times()' first value)."""
        a = C.c_double()
        self._L.g1s_denoise_level_time(self._h, C.byref(a))
        return a.value

    def level_kernel_time(self) -> float:
        """ms in kd_down, kd_lowres and kd_add alone, every level's, of the timed batches so far (a part of level_time())."""
        a = C.c_double()
        self._L.g1s_denoise_level_kernel_time(self._h, C.byref(a))
        return a.value

    def kernel_times(self, enable: bool = True):
        """(ms in kd_nlm and kd_nlm_j, whichever form -- with a curve also the two kd_curve launches -- , frames) of the timed batches
        so far (HIP events); enables / disables the timing."""
        a, n = C.c_double(), C.c_uint64()
        self._L.g1s_denoise_set_timing(self._h, int(enable), C.byref(a), C.byref(n))
        return a.value, n.value


def denoise_y4m_file(input: str, output: str, *, device: int = -1, batch_frames: int = 0, search_radius: int = 0, patch_radius: int = 0,
                     strength: float = 0.0, chroma_strength: float = 0.0, temporal_radius: int = 0, joint_chroma: bool = False,
                     grain_prior: Optional[str] = None, prior_range: int = 0, prior_segment: Optional[int] = None, motion_range: int = 0,
                     auto_prior: bool = False, auto_strength: bool = False, profile_frames: int = 0, levels_min_count: int = 0,
                     chroma_prior: bool = False, coarse_levels: int = 0, coarse_ratio: float = 0.0, auto_temporal: bool = False) -> int:
    """`denoise INPUT -o OUTPUT` for a .y4m input; the file is one clip.  grain_prior: a grain table whose luma scaling
    function the luma strength follows (grain_curve() with prior_range and prior_segment).  motion_range: as Denoiser takes
    it.  auto_prior / auto_strength: the curve and the strengths from the clip's own noise levels (rules N5 - N7), measured
    in a pre-pass over its first profile_frames frames (0 = all) with levels_min_count as Nmin (0 = 4096).  chroma_prior: the
    job's prior also gives the joint chroma filter its gain (rules 21 - 24): from the table's chroma scaling functions, or from
    the chroma levels the pre-pass measured; needs joint_chroma and one of grain_prior / auto_prior.  coarse_levels, coarse_ratio: as
    Denoiser takes them; an auto strength is level 0's.  auto_temporal: the pre-pass measures temporal noise levels (rules T1 -
    T7: the difference of consecutive frames, which holds on correlated grain) and the auto values are T7's; needs auto_prior or
    auto_strength and a pre-pass of two frames.  Returns the number of frames."""
    L = _lib.lib()
    opts = denoise_opts(device, batch_frames, search_radius, patch_radius, strength, chroma_strength)
    err = C.create_string_buffer(512)
    if grain_prior is None and (prior_range or prior_segment is not None):
        raise G1SError(-1, "prior_range and prior_segment need grain_prior")
    prior = (str(grain_prior).encode() if grain_prior is not None else None, prior_range & 0xFFFFFFFF, -1 if prior_segment is None else prior_segment)
    auto = (_lib.G1S_AUTO_PRIOR if auto_prior else 0) | (_lib.G1S_AUTO_STRENGTH if auto_strength else 0)
    args = (input.encode(), output.encode(), C.byref(opts), temporal_radius & 0xFFFFFFFF, _flags(joint_chroma), *prior, motion_range & 0xFFFFFFFF, auto,
            profile_frames, levels_min_count, 1 if chroma_prior else 0, coarse_levels & 0xFFFFFFFF, float(coarse_ratio))
    if auto_temporal:
        n = L.g1s_denoise_y4m_file_auto_temporal(*args, 1, err, len(err))
    else:
        n = L.g1s_denoise_y4m_file_levels(*args, err, len(err))
    if n < 0:
        raise G1SError(int(n), err.value.decode())
    log.info("Denoised %d frames", n)
    return int(n)
