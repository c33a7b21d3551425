"""`render` on the device against the numpy restatement of the standard (tests/grain_ref.py): every template entry, every
table entry and every rendered sample equal, byte for byte."""
from __future__ import annotations

import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from grav1synth_amd.diff import DEFAULT_GRAIN_SEED, GrainTableSegment
from tests import grain_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBSAMPLINGS = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}


def make_segment(lag=3, seed=1234, *, rng=None, num_y=3, num_cb=2, num_cr=4, scaling_shift=9, ar_shift=7, grain_scale_shift=0,
                 overlap=True, csfl=False, mults=(128, 192, 256, 120, 200, 250)) -> GrainTableSegment:
    """A parameter set with a stable AR filter (small taps far from the sample, the energy next to it)."""
    rng = rng or np.random.default_rng(seed * 7 + lag)
    n = 2 * lag * (lag + 1)

    def coeffs(extra):
        c = rng.integers(-12, 13, n + extra)
        if n:
            c[n - 1] = 50  # the left neighbour
            if lag >= 1:
                c[n - 1 - (lag + 1)] = 30  # the sample above
        if extra:
            c[n] = int(rng.integers(-60, 61))
        return [int(v) for v in c]

    def points(k, lo, hi):
        xs = sorted(rng.choice(np.arange(1, 255), size=max(k - 2, 0), replace=False).tolist())
        xs = ([0] + xs + [255])[:k] if k >= 2 else [int(rng.integers(0, 256))][:k]
        return [(int(x), int(rng.integers(lo, hi))) for x in xs]

    return GrainTableSegment(
        random_seed=seed, start_time=0, end_time=2 ** 63 - 1,
        scaling_points_y=points(num_y, 20, 120), scaling_points_cb=points(num_cb, 10, 255), scaling_points_cr=points(num_cr, 0, 90),
        scaling_shift=scaling_shift, ar_coeff_lag=lag, ar_coeffs_y=coeffs(0), ar_coeffs_cb=coeffs(1), ar_coeffs_cr=coeffs(1),
        ar_coeff_shift=ar_shift, cb_mult=mults[0], cb_luma_mult=mults[1], cb_offset=mults[2], cr_mult=mults[3],
        cr_luma_mult=mults[4], cr_offset=mults[5], chroma_scaling_from_luma=csfl, grain_scale_shift=grain_scale_shift,
        overlap_flag=overlap)


def content(w, h, bd, subx, suby, seed=0, mono=False, kind="noise"):
    """Full-range planes: random samples, or all 0 / all max / a ramp so that every clip is exercised."""
    rng = np.random.default_rng(seed + w * 31 + h)
    top = (1 << bd) - 1
    dt = np.uint8 if bd == 8 else np.uint16
    shapes = [(h, w)] + ([] if mono else [((h + suby) >> suby, (w + subx) >> subx)] * 2)
    out = []
    for i, s in enumerate(shapes):
        if kind == "noise":
            p = rng.integers(0, top + 1, s)
        elif kind == "zero":
            p = np.zeros(s, np.int64)
        elif kind == "max":
            p = np.full(s, top)
        else:  # ramp
            p = (np.arange(s[0] * s[1]).reshape(s) * (7 + i)) % (top + 1)
        out.append(p.astype(dt))
    return out


def assert_planes_equal(got, want, what):
    assert len(got) == len(want)
    for c, (a, b) in enumerate(zip(got, want)):
        a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what} plane {c}: {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
        bad = np.argwhere(a != b)
        assert len(bad) == 0, f"{what} plane {c}: {len(bad)} samples differ, first at {bad[0].tolist()}: {a[tuple(bad[0])]} vs {b[tuple(bad[0])]}"


@pytest.fixture(scope="module")
def synths():
    from grav1synth_amd.grain import GrainSynthesizer

    made = {}

    def get(bd, **kw):
        key = (bd, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = GrainSynthesizer(bd, **kw)
        return made[key]

    yield get
    for s in made.values():
        s.close()


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("ss", ["420", "422", "444"])
def test_templates_and_tables_equal_the_standard(synths, bd, ss):
    subx, suby = SUBSAMPLINGS[ss]
    from grav1synth_amd.grain import GrainSynthesizer

    syn = GrainSynthesizer(bd)  # (its own: the templates call must work before any frame has set a geometry)
    seeds = [0, 0xFFFF, 1, 10956, 0x8000]
    k = 0
    for lag in range(4):
        for gss in range(4):
            seed = seeds[k % len(seeds)]
            k += 1
            seg = make_segment(lag, seed, grain_scale_shift=gss, num_y=2 + lag, num_cb=lag, num_cr=5, ar_shift=6 + (k % 4))
            luma, cb, cr, lut = syn.templates(seg, subx, suby)
            rl, rcb, rcr = R.generate_grain(seg, bd, subx, suby)
            what = f"lag {lag} gss {gss} seed {seed} {bd} bit {ss}"
            assert np.array_equal(luma, rl), what + ": luma template"
            assert np.array_equal(cb, rcb), what + ": cb template"
            assert np.array_equal(cr, rcr), what + ": cr template"
            assert np.array_equal(lut, R.scaling_luts(seg)), what + ": scaling tables"
    for seed in seeds:  # every seed at lag 3
        seg = make_segment(3, seed)
        luma, cb, cr, lut = syn.templates(seg, subx, suby)
        rl, rcb, rcr = R.generate_grain(seg, bd, subx, suby)
        assert np.array_equal(luma, rl) and np.array_equal(cb, rcb) and np.array_equal(cr, rcr), f"seed {seed}"
    syn.close()


def test_templates_with_luma_scaling_for_chroma_and_without_luma_points(synths):
    syn = synths(10)
    for seg in (make_segment(2, 77, csfl=True, num_cb=0, num_cr=0), make_segment(3, 78, num_y=0), make_segment(1, 79, num_y=1, num_cb=1, num_cr=1)):
        luma, cb, cr, lut = syn.templates(seg, 1, 1)
        rl, rcb, rcr = R.generate_grain(seg, 10, 1, 1)
        assert np.array_equal(luma, rl) and np.array_equal(cb, rcb) and np.array_equal(cr, rcr)
        assert np.array_equal(lut, R.scaling_luts(seg))


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("ss", ["420", "422", "444"])
def test_rendered_planes_equal_the_standard(synths, bd, ss):
    subx, suby = SUBSAMPLINGS[ss]
    syn = synths(bd)
    w, h = 320, 192
    k = 0
    for lag in range(4):
        for overlap in (False, True):
            seg = make_segment(lag, 100 + k, overlap=overlap, grain_scale_shift=k % 4, scaling_shift=8 + k % 4)
            k += 1
            planes = content(w, h, bd, subx, suby, seed=k)
            dev = _to_dev(planes, bd)
            got = syn.apply(dev, seg, subx, suby)
            assert_planes_equal(got, R.add_noise(planes, seg, bd, subx, suby), f"lag {lag} overlap {overlap} {bd} bit {ss}")
            assert_planes_equal(dev, planes, "the input planes after the call")


def _to_dev(planes, bd):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(p)).to("cuda") for p in planes]


SIZE_CASES = [(size, bd, ss) for size in [(322, 194), (35, 33), (321, 193)] for bd, ss in [(8, "420"), (10, "420"), (10, "422"), (12, "444")]]
SIZE_CASES += [((1920, 1080), 8, "420"), ((1920, 1080), 10, "420")]


@pytest.mark.parametrize("size,bd,ss", SIZE_CASES)
def test_sizes_that_are_not_multiples_of_the_block(synths, size, bd, ss):
    subx, suby = SUBSAMPLINGS[ss]
    w, h = size
    seg = make_segment(3, w + h + bd)
    planes = content(w, h, bd, subx, suby)
    got = synths(bd).apply(_to_dev(planes, bd), seg, subx, suby)
    assert_planes_equal(got, R.add_noise(planes, seg, bd, subx, suby), f"{w}x{h} {bd} bit {ss}")


def test_4k_10_bit(synths):
    seg = make_segment(3, 4000)
    planes = content(3840, 2160, 10, 1, 1)
    got = synths(10).apply(_to_dev(planes, 10), seg, 1, 1)
    assert_planes_equal(got, R.add_noise(planes, seg, 10, 1, 1), "3840x2160")


@pytest.mark.parametrize("bd", [8, 10])
def test_parameter_corners(synths, bd):
    w, h = 320, 192
    cases = {
        "chroma_scaling_from_luma": make_segment(2, 1, csfl=True),
        "csfl without chroma points": make_segment(2, 2, csfl=True, num_cb=0, num_cr=0),
        "no luma points, chroma present": make_segment(3, 3, num_y=0),
        "no cb points": make_segment(3, 4, num_cb=0),
        "no points at all": make_segment(3, 5, num_y=0, num_cb=0, num_cr=0),
        "one point": make_segment(1, 6, num_y=1, num_cb=1, num_cr=1),
        "fourteen points": make_segment(3, 7, num_y=14, num_cb=10, num_cr=10),
        "extreme chroma mults": make_segment(3, 8, mults=(255, 0, 511, 0, 255, 0)),
    }
    for name, seg in cases.items():
        for kind in ("noise", "zero", "max", "ramp"):
            planes = content(w, h, bd, 1, 1, kind=kind)
            got = synths(bd).apply(_to_dev(planes, bd), seg, 1, 1)
            assert_planes_equal(got, R.add_noise(planes, seg, bd, 1, 1), f"{name} / {kind} / {bd} bit")


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("mc_identity", [False, True])
def test_clip_to_restricted_range(synths, bd, mc_identity):
    seg = make_segment(3, 9, scaling_shift=8)
    for kind in ("noise", "zero", "max"):
        planes = content(320, 192, bd, 1, 1, kind=kind)
        got = synths(bd, clip_to_restricted_range=True, mc_identity=mc_identity).apply(_to_dev(planes, bd), seg, 1, 1)
        want = R.add_noise(planes, seg, bd, 1, 1, clip_to_restricted_range=True, mc_identity=mc_identity)
        assert_planes_equal(got, want, f"restricted range, identity {mc_identity}, {kind}")
    # a plane without points is copied, not clipped
    seg = make_segment(3, 10, num_cb=0)
    planes = content(320, 192, bd, 1, 1, kind="max")
    got = synths(bd, clip_to_restricted_range=True, mc_identity=mc_identity).apply(_to_dev(planes, bd), seg, 1, 1)
    assert_planes_equal(got, R.add_noise(planes, seg, bd, 1, 1, clip_to_restricted_range=True, mc_identity=mc_identity), "no cb points")


def test_monochrome_and_no_segment(synths):
    seg = make_segment(3, 11)
    planes = content(322, 194, 10, 0, 0, mono=True)
    got = synths(10).apply(_to_dev(planes, 10), seg, 0, 0)
    assert_planes_equal(got, R.add_noise(planes, seg, 10, 0, 0), "monochrome")
    planes = content(322, 194, 8, 1, 1)
    got = synths(8).apply(_to_dev(planes, 8), None, 1, 1)
    assert_planes_equal(got, planes, "no segment: a copy")


def test_strided_device_tensors_and_host_pinned_device_frames_agree(synths):
    import torch

    from grav1synth_amd import _lib
    from grav1synth_amd.diff import Frame

    bd, (subx, suby) = 10, (1, 1)
    w, h = 322, 194
    seg = make_segment(3, 12)
    planes = content(w, h, bd, subx, suby)
    want = R.add_noise(planes, seg, bd, subx, suby)
    syn = synths(bd)
    # rows wider than the plane, starting off a 16-byte boundary
    strided_in, strided_out, out_bases = [], [], []
    for p in planes:
        big = np.zeros((p.shape[0], p.shape[1] + 13), np.uint16)
        big[:, 3:3 + p.shape[1]] = p
        strided_in.append(torch.from_numpy(big).to("cuda")[:, 3:3 + p.shape[1]])
        obig = torch.from_numpy(np.full((p.shape[0], p.shape[1] + 9), 0xABCD, np.uint16)).to("cuda")
        out_bases.append(obig)
        strided_out.append(obig[:, 5:5 + p.shape[1]])
    got = syn.apply(strided_in, seg, subx, suby, out=strided_out)
    assert_planes_equal(got, want, "strided device tensors")
    for o, base in zip(strided_out, out_bases):  # nothing written outside the plane's columns
        full = base.cpu().numpy()
        assert (full[:, :5] == 0xABCD).all() and (full[:, 5 + o.shape[1]:] == 0xABCD).all()
    # host (numpy) frames
    assert_planes_equal(syn.apply(planes, seg, subx, suby), want, "host frames")
    # pinned host frames through the C ABI (on_device = 2), input and output
    L = _lib.lib()
    pin_in = [torch.from_numpy(np.ascontiguousarray(p)).pin_memory() for p in planes]
    pin_out = [torch.from_numpy(np.zeros(p.shape, np.uint16)).pin_memory() for p in planes]
    keep = []
    fin = Frame(pin_in, subx, suby, async_host=True).to_c(keep)
    fout = Frame(pin_out, subx, suby, async_host=True).to_c(keep)
    assert fin.on_device == 2 and fout.on_device == 2
    import ctypes as C

    c_seg = seg.to_c()
    assert L.g1s_grain_frame(syn._h, C.byref(c_seg), C.byref(fin), C.byref(fout)) == 0
    syn.sync()
    assert_planes_equal([p.numpy() for p in pin_out], want, "pinned frames")
    # in == out is refused (and the refusal is sticky: a synthesizer of its own)
    from grav1synth_amd.grain import GrainSynthesizer

    own = GrainSynthesizer(bd)
    dev = _to_dev(planes, bd)
    with pytest.raises(_lib.G1SError) as e:
        own.apply(dev, seg, subx, suby, out=dev)
    assert "distinct" in str(e.value)
    own.close()


def test_a_batch_of_70_frames_equals_70_single_calls(synths):
    from grav1synth_amd.grain import GrainSynthesizer

    bd, (subx, suby) = 8, (1, 1)
    w, h = 162, 98
    segs = [make_segment(3, 21), make_segment(1, 22, overlap=False), make_segment(2, 23, csfl=True)]
    batched = GrainSynthesizer(bd, batch_frames=32)
    single = synths(bd)
    outs, wants, ins = [], [], []
    for k in range(70):
        seg = None if k == 40 else segs[(k // 9) % 3]
        if seg is not None:
            seg = GrainTableSegment(**{**seg.__dict__, "random_seed": (seg.random_seed + DEFAULT_GRAIN_SEED * (k + 1)) & 0xFFFF})
        planes = content(w, h, bd, subx, suby, seed=k)
        dev = _to_dev(planes, bd)
        ins.append(dev)
        outs.append(batched.apply(dev, seg, subx, suby, sync=False))
        wants.append(single.apply(dev, seg, subx, suby))
        if k in (0, 33, 69):  # ... and the single calls are the standard's
            assert_planes_equal(wants[-1], R.add_noise(planes, seg, bd, subx, suby) if seg else planes, f"frame {k}")
    batched.sync()
    for k in range(70):
        assert_planes_equal(outs[k], [p.cpu().numpy() for p in wants[k]], f"batched frame {k}")
    batched.close()


def _diff_table(tmp_path, frames_spec):
    """A table made by the device `diff` on the repository's synthetic content, with a scene cut."""
    import torch  # noqa: F401

    from grav1synth_amd.diff import DiffGenerator
    from grav1synth_amd.synth import SynthSpec, make_pair

    spec_a, spec_b, n = frames_spec
    g = DiffGenerator(Fraction(24, 1), spec_a.bit_depth, spec_a.bit_depth, device=0)
    for k in range(n):
        sp = spec_a if k < n // 2 else spec_b
        s, d = make_pair(sp, k, device="cuda:0")
        g.diff_frame(s, d, sp.xdec, sp.ydec)
    return g.finish()


def test_frames_on_both_sides_of_a_scene_cut_take_their_own_segment(synths, tmp_path):
    from grav1synth_amd.ingest import write_y4m
    from grav1synth_amd.diff import format_tbl
    from grav1synth_amd.grain import render_y4m_file
    from grav1synth_amd.ingest import Y4MReader
    from grav1synth_amd.synth import SynthSpec, make_pair
    from grav1synth_amd.tbl import GrainTable

    a = SynthSpec(320, 192, 8)
    b = SynthSpec(320, 192, 8, gain_scale=2)  # (the scene-cut variant: twice the noise gain)
    n = 8
    segs = _diff_table(tmp_path, (a, b, n))
    assert len(segs) >= 2, "the content change did not cut the table"
    tbl = tmp_path / "cut.tbl"
    tbl.write_bytes(format_tbl(segs))
    clean = []
    for k in range(n):
        _, d = make_pair(a if k < n // 2 else b, k, device="cpu")
        clean.append([p.numpy() for p in d])
    src = tmp_path / "clean.y4m"
    write_y4m(str(src), clean, 8, 1, 1, Fraction(24, 1))
    out = tmp_path / "grainy.y4m"
    assert render_y4m_file(str(src), str(tbl), str(out)) == n
    table = GrainTable(segs)
    rd = Y4MReader(str(out))
    used = set()
    for k in range(n):
        ts = k * 10000000 * 1 // 24
        seg = table.segment_for(ts)
        assert seg is not None
        used.add(seg.start_time)
        got = rd.get_frame()
        assert_planes_equal([np.asarray(p) for p in got], R.add_noise(clean[k], seg, 8, 1, 1), f"frame {k}")
    assert rd.get_frame() is None
    rd.close()
    assert len(used) >= 2


def test_render_command_end_to_end(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_y4m_fixture as fx

    from grav1synth_amd.ingest import Y4MReader
    from grav1synth_amd.tbl import GrainTable, parse_tbl

    fx.main(str(tmp_path))
    name = "320x200_10b_420"
    spec, fps, _src, den = fx.frames_of(name)
    clean = tmp_path / (name + "_denoised.y4m")
    tbl = os.path.join(ROOT, "tests", "golden", "oracle_320x200_10b_420_lag3.tbl")
    out = tmp_path / "grainy.y4m"
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "grav1synth_amd", "render", str(clean), "-g", tbl, "-o", str(out)]
    p = subprocess.run(cmd + ["-y"], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert f"Done, wrote output file to {out}" in p.stderr
    assert open(out, "rb").readline() == open(clean, "rb").readline(), "the output's header is the input's"
    table = GrainTable(parse_tbl(open(tbl, "rb").read()))
    rd = Y4MReader(str(out))
    for k, planes in enumerate(den):
        seg = table.segment_for(k * 10000000 * fps.denominator // fps.numerator)
        want = R.add_noise(planes, seg, spec.bit_depth, spec.xdec, spec.ydec) if seg else planes
        assert_planes_equal([np.asarray(q) for q in rd.get_frame()], want, f"frame {k}")
    assert rd.get_frame() is None
    rd.close()
    # the refusals: output equal to an input; an existing output without -y (no terminal: an error exit, as diff's)
    before = open(out, "rb").read()
    p = subprocess.run(cmd[:-1] + [str(clean)], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0 and "Input and output paths are the same" in p.stderr
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT, stdin=subprocess.DEVNULL)
    assert p.returncode == 1 and "not a terminal" in p.stderr
    assert open(out, "rb").read() == before


def test_closed_loop_on_the_device():
    """GrainSynthesizer -> DiffGenerator: known parameters rendered on the device, estimated on the device, compared within the
    bounds of the CPU loop (tests/test_grain_cpu.py: what is compared, and what was observed)."""
    from grav1synth_amd.diff import DiffGenerator
    from grav1synth_amd.grain import GrainSynthesizer
    from tests.test_grain_cpu import AR_BOUND, CY3, STD_BOUND, segment, smooth_frame

    bd, (subx, suby), lag, cy = 10, (1, 1), 3, CY3
    pts_y, pts_c = [(0, 30), (64, 50), (128, 60), (192, 50), (255, 70)], [(0, 30), (255, 60)]
    cc = [c // 2 for c in cy] + [40]
    clean = _to_dev(smooth_frame(640, 384, bd, subx, suby), bd)
    syn = GrainSynthesizer(bd)
    differ = DiffGenerator(Fraction(24, 1), bd, bd, ar_coeff_lag=lag, device=0)
    for k in range(6):
        seg = segment(lag, cy, cc, pts_y, pts_c, (7391 + 10956 * (k + 1)) & 0xFFFF)
        differ.diff_frame(syn.apply(clean, seg, subx, suby), clean, subx, suby)
    emitted = differ.finish()
    syn.close()
    assert emitted
    n = 2 * lag * (lag + 1)
    want = np.array(cy) / 2.0 ** 7
    xs = np.arange(40, 200, 16)
    true_std = R.scaling_lut(pts_y)[xs] / 2.0 ** 8 * R.generate_grain(seg, bd, subx, suby, mono=True)[0][9:, 9:].std()
    for e in emitted:
        got = np.array(e.ar_coeffs_y[:n]) / 2.0 ** e.ar_coeff_shift
        assert np.abs(got - want).max() <= AR_BOUND, (e.ar_coeffs_y, e.ar_coeff_shift)
        back = segment(lag, list(e.ar_coeffs_y[:n]), list(e.ar_coeffs_y[:n]) + [0], e.scaling_points_y, [], 1,
                       scaling_shift=e.scaling_shift, ar_shift=e.ar_coeff_shift)
        est_std = R.scaling_lut(e.scaling_points_y)[xs] / 2.0 ** e.scaling_shift * R.generate_grain(back, bd, subx, suby, mono=True)[0][9:, 9:].std()
        assert np.abs(est_std / true_std - 1).max() <= STD_BOUND, (e.scaling_points_y, e.scaling_shift)
