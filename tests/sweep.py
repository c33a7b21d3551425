"""Seeded, edge-biased case lists for every device operation, and the inputs a case stands for (test infrastructure).

`cases(op, seed, n)` returns `n` plain records (dicts of ints, floats, strings, bools and lists of those) drawn from
`numpy.random.default_rng([seed, op_id])`: the same arguments give the same list on every machine, and a record printed by a
failing test can be pasted back (`eval(repr(case)) == case`; `tools/fuzz_parity.py OP --case 'RECORD'`).  Every axis is
drawn from a menu weighted towards the places kernels go wrong -- one below, on and one above a tile, block or unit edge,
parameter extremes, clips shorter than their window, frame counts around a batch -- and the record carries the name of the
menu entry it took (`wc`, `hc`, `nc`, ...), which is what tests/test_sweep_cpu.py counts.  The first records of an operation
are fixed corner cases (`forced`): crossings a short list must not leave to chance.

The second half of the file turns a record into its inputs (numpy only, no device): `segment_of`, `render_planes`,
`denoise_frames`, `estimate_plane`, `resize_planes_of`, `diff_frames`.  tests/test_gpu_sweep.py runs them on the device and
against the references; SUITE is the committed (seed, n, chunks) per operation.
"""
from __future__ import annotations

import hashlib
from typing import Dict, List, Tuple

import numpy as np

OPS = ("diff", "render", "denoise", "denoise_t", "estimate", "resize")
# (seed, cases, chunks): what `pytest tests -m gpu` runs.  tools/fuzz_parity.py takes the same generator further.
SUITE: Dict[str, Tuple[int, int, int]] = {
    "diff": (12, 56, 8),
    "render": (12, 72, 6),
    "denoise": (12, 80, 4),
    "denoise_t": (12, 48, 6),
    "estimate": (12, 96, 2),
    "resize": (12, 120, 3),
}
SUBSAMPLINGS = {"420": (1, 1), "422": (1, 0), "444": (0, 0), "mono": (0, 0)}
ALGS = ("hermite", "catmullrom", "mitchell", "lanczos", "spline36")
KSLOTS = 6  # batches in flight in the diff engine: batch j runs in slot j % 6


def _pick(rng, menu):
    """One entry of [(value, weight), ...]."""
    w = np.array([m[1] for m in menu], float)
    return menu[int(rng.choice(len(menu), p=w / w.sum()))][0]


def _edge(rng, unit: int, kmax: int, uni: Tuple[int, int], small=True, kmin=1, plus2=False):
    """(size, class): 1, 2, 3, k unit - 1, k unit, k unit + 1 (and + 2), or a uniform remainder."""
    menu = [("ku-1", 3), ("ku", 3), ("ku+1", 3), ("uni", 3)]
    if small:
        menu += [("1", 0.5), ("2", 0.5), ("3", 0.5)]
    if plus2:
        menu += [("ku+2", 2)]
    c = _pick(rng, menu)
    k = int(rng.integers(kmin, kmax + 1))
    if c in ("1", "2", "3"):
        return int(c), c
    if c == "uni":
        return int(rng.integers(uni[0], uni[1] + 1)), c
    return k * unit + {"ku-1": -1, "ku": 0, "ku+1": 1, "ku+2": 2}[c], c


def _cls(v: int, unit: int, plus2=False) -> str:
    """The class of _edge a given size falls in (the fixed corner cases are counted like the drawn ones)."""
    if v <= 3:
        return str(v)
    r = v % unit
    return "ku" if r == 0 else "ku+1" if r == 1 and v > unit else "ku-1" if r == unit - 1 else "ku+2" if r == 2 and v > unit and plus2 else "uni"


def digest(case_list) -> str:
    """SHA-256 of the list as it prints."""
    return hashlib.sha256(repr(case_list).encode()).hexdigest()


def chunk_of(case_list, chunk: int, chunks: int):
    return case_list[chunk::chunks]  # (strided: the forced cases at the head are shared out)


def suite_cases(op: str):
    seed, n, _chunks = SUITE[op]
    return cases(op, seed, n)


def cases(op: str, seed: int, n: int) -> List[dict]:
    if op not in OPS:
        raise ValueError(f"unknown operation {op!r}: one of {', '.join(OPS)}")
    rng = np.random.default_rng([seed, OPS.index(op)])
    draw = globals()["_draw_" + op]
    forced = globals()["_FORCED_" + op.upper()]
    if op in ("denoise", "denoise_t"):
        pool = _dn_pool(rng, op == "denoise_t")
        draw = lambda r, _d=draw: _d(r, pool)  # noqa: E731
    out = []
    for i in range(n):
        c = dict(forced[i]) if i < len(forced) else draw(rng)
        c = {"op": op, "i": i, **c}
        c.setdefault("forced", i < len(forced))
        out.append(c)
    return out


# ---- diff ---------------------------------------------------------------------------------------------------------------

DEPTH_PAIRS = [((8, 8), 3), ((10, 10), 3), ((12, 12), 2), ((10, 8), 1), ((8, 10), 1), ((12, 10), 1), ((10, 12), 1)]
# (blocks, width, height): luma-only 8-bit frames around k4_latest's 1024-block chunks and the 4 096 blocks from which the
# device half of the fold is the default
BLOCK_GEOMS = [(1023, 33 * 32, 31 * 32), (1024, 1024, 1024), (1025, 41 * 32, 25 * 32), (2047, 23 * 32, 89 * 32), (2048, 2048, 1024),
               (4095, 63 * 32, 65 * 32), (4096, 2048, 2048), (4097, 17 * 32, 241 * 32)]


def _diff_big(blocks: int, latest: str, cut_last=0, nframes=2, batch=2, where="device", lag=3, textured=False) -> dict:
    _b, w, h = next(g for g in BLOCK_GEOMS if g[0] == blocks)
    return dict(w=w - cut_last, h=h, wc="blocks", hc="blocks", blocks=blocks, src_bd=8, den_bd=8, ss="420", lag=lag, chroma=False,
                content="synth", kinds=[], textured=textured, nframes=nframes, batch=batch, nc="kb", cut=-1, cutc="none", k3="", latest=latest,
                where=where, cseed=blocks)


_FORCED_DIFF = [
    # (the oracle pays about a second per thousand blocks and frame at lag 3: one frame, or a shorter lag, where the block count is the point;
    # whole blocks up to the right edge where a chunk's last block must count: cut at the edge, block 1 024 of 1 025 was not measured on this content)
    _diff_big(1024, "device"), _diff_big(1025, "device"), _diff_big(2047, "device", lag=2, textured=True), _diff_big(1023, "device", lag=1),
    _diff_big(4095, "", nframes=1, batch=1), _diff_big(4096, "", cut_last=31, lag=2), _diff_big(4097, "", nframes=1, lag=1),
    _diff_big(4096, "host", nframes=1, batch=1), _diff_big(2048, "device", batch=1), _diff_big(1025, "host", cut_last=9, where="host", lag=2, textured=True),
]


def _draw_diff(rng) -> dict:
    ss = _pick(rng, [("420", 4), ("422", 2), ("444", 2)])
    xd, _yd = SUBSAMPLINGS[ss]
    s = 16 << xd  # a multiple of 16 samples in every plane
    wc = _pick(rng, [("32k-1", 2), ("32k", 2), ("32k+1", 2), ("128k", 2), ("128k+16", 2), ("128k-16", 2), ("16m", 2), ("16m+8", 1),
                     ("16m+1", 1), ("16m-1", 1), ("66", 0.5), ("67", 0.5), ("uni", 3)])
    k = int(rng.integers(3, 10))
    m = int(rng.integers(5, 288 // s + 1))
    w = {"32k-1": 32 * k - 1, "32k": 32 * k, "32k+1": 32 * k + 1, "128k": 128 * int(rng.integers(1, 4)),
         "128k+16": 128 * int(rng.integers(1, 3)) + s, "128k-16": 128 * int(rng.integers(1, 4)) - s, "16m": s * m, "16m+8": s * m + s // 2,
         "16m+1": s * m + 1, "16m-1": s * m - 1, "66": 66, "67": 67, "uni": int(rng.integers(66, 301))}[wc]
    hc = _pick(rng, [("32k-1", 2), ("32k", 2), ("32k+1", 2), ("66", 0.5), ("67", 0.5), ("uni", 3)])
    k = int(rng.integers(3, 8))
    h = {"32k-1": 32 * k - 1, "32k": 32 * k, "32k+1": 32 * k + 1, "66": 66, "67": 67, "uni": int(rng.integers(66, 221))}[hc]
    src_bd, den_bd = _pick(rng, DEPTH_PAIRS)
    batch = int(rng.integers(1, 6))
    nc = _pick(rng, [("kb-1", 2), ("kb", 2), ("kb+1", 2), ("ring", 1.5)])
    kb = int(rng.integers(1, 4))
    nframes = {"kb-1": kb * batch - 1, "kb": kb * batch, "kb+1": kb * batch + 1, "ring": (KSLOTS + 1) * min(batch, 2) + int(rng.integers(0, 2))}[nc]
    if nc == "ring":
        batch = min(batch, 2)
    nframes = max(nframes, 1)
    content = _pick(rng, [("content", 3), ("synth", 2)])
    kinds = [str(_pick(rng, [("distinct", 3), ("flat", 2), ("busy", 1), ("damaged", 2), ("clamped", 1)])) for _ in range(nframes)] if content == "content" else []
    cut, cutc = -1, "none"
    if content == "synth" and nframes >= 2:
        cutc = _pick(rng, [("none", 2), ("edge", 2), ("inside", 2)])
        edges = [f for f in range(1, nframes) if f % batch == 0]
        inside = [f for f in range(1, nframes) if f % batch != 0]
        pool = edges if cutc == "edge" else inside if cutc == "inside" else []
        if pool:
            cut = int(pool[int(rng.integers(0, len(pool)))])
        else:
            cutc = "none"
    return dict(w=w, h=h, wc=wc, hc=hc, blocks=((w + 31) // 32) * ((h + 31) // 32), src_bd=src_bd, den_bd=den_bd, ss=ss,
                lag=int(_pick(rng, [(1, 1), (2, 1), (3, 2)])), chroma=bool(rng.random() < 0.75), content=content, kinds=kinds,
                textured=bool(rng.random() < 0.6), nframes=nframes, batch=batch, nc=nc, cut=cut, cutc=cutc,
                k3=_pick(rng, [("", 5), ("stream", 1)]), latest=_pick(rng, [("", 2), ("host", 2), ("device", 3)]),
                where=_pick(rng, [("device", 3), ("host", 1)]), cseed=int(rng.integers(0, 1 << 16)))


def diff_frames(c: dict):
    """[(source planes, denoised planes)] of a diff case: host numpy planes, chroma dropped for a luma-only case."""
    from grav1synth_amd.synth import SynthSpec, make_pair
    from tests.content import make_frames

    xd, yd = SUBSAMPLINGS[c["ss"]]
    out = []
    for f in range(c["nframes"]):
        if c["content"] == "content":
            s = make_frames(c["kinds"][f], c["w"], c["h"], c["src_bd"], xd, yd, f, seed=c["cseed"])[0]
            d = make_frames(c["kinds"][f], c["w"], c["h"], c["den_bd"], xd, yd, f, seed=c["cseed"])[1]
        else:
            gain = 3 if 0 <= c["cut"] <= f else 1
            kw = dict(xdec=xd, ydec=yd, textured=c["textured"], gain_scale=gain, nplanes=3 if c["chroma"] else 1)
            s = [p.numpy() for p in make_pair(SynthSpec(c["w"], c["h"], c["src_bd"], **kw), f)[0]]
            d = [p.numpy() for p in make_pair(SynthSpec(c["w"], c["h"], c["den_bd"], **kw), f)[1]]
        if not c["chroma"]:
            s, d = s[:1], d[:1]
        out.append((s, d))
    return out


# ---- render -------------------------------------------------------------------------------------------------------------

GRAIN_SEEDS = [(0, 1), (1, 1), (0x8000, 1), (0xFFFF, 1), (1 << 11, 0.4), (1 << 12, 0.4), (1 << 13, 0.4), (1 << 14, 0.4), (1 << 15, 0.4), ("uni", 3)]


def _render(w, h, bd, ss, lag, **kw) -> dict:
    c = dict(w=w, h=h, wc=_cls(w, 32, True), hc=_cls(h, 32, True), bd=bd, ss=ss, lag=lag, ar_shift=7, gss=0, scaling_shift=9, num_y=3, num_cb=2, num_cr=4,
             points="ends", coeffs="stable", csfl=False, overlap=True, mults=[128, 192, 256, 120, 200, 250], seed=1234, clip=False,
             mc_identity=False, kind="noise", sseed=w * 131 + h)
    c.update(kw)
    return c


_FORCED_RENDER = [
    # the overlap blend where the last block has one or two columns / rows, in every subsampling
    _render(65, 33, 8, "420", 3), _render(33, 65, 10, "420", 2), _render(66, 34, 12, "422", 3), _render(97, 33, 10, "444", 1),
    _render(34, 66, 8, "444", 3), _render(33, 33, 10, "422", 0),
    # templates that saturate at both ends of the grain range
    _render(70, 40, 8, "420", 3, coeffs="full", ar_shift=6, seed=0xFFFF), _render(40, 70, 12, "444", 2, coeffs="full", ar_shift=6, gss=0, seed=0x8000),
    _render(1, 1, 10, "420", 3), _render(2, 3, 8, "422", 1), _render(3, 2, 12, "mono", 2),
    _render(64, 64, 10, "420", 3, clip=True, mc_identity=True, kind="max", num_y=14, num_cb=10, num_cr=10, points="equal_y"),
    _render(95, 31, 8, "420", 3, csfl=True, num_cb=0, num_cr=0, kind="ramp", mults=[255, 0, 511, 0, 255, 0]),
]


def _draw_render(rng) -> dict:
    ss = _pick(rng, [("420", 4), ("422", 2), ("444", 2), ("mono", 1)])
    w, wc = _edge(rng, 32, 5, (4, 200), plus2=True)
    h, hc = _edge(rng, 32, 4, (4, 150), plus2=True)
    seed = _pick(rng, GRAIN_SEEDS)
    npts = [(0, 1), (1, 1), (2, 2), (10, 2), (14, 1), ("uni", 2)]

    def count(cap):
        v = _pick(rng, npts)
        return min(int(rng.integers(3, cap + 1)) if v == "uni" else v, cap)

    return dict(w=w, h=h, wc=wc, hc=hc, bd=int(_pick(rng, [(8, 1), (10, 1), (12, 1)])), ss=ss, lag=int(rng.integers(0, 4)),
                ar_shift=int(rng.integers(6, 10)), gss=int(rng.integers(0, 4)), scaling_shift=int(rng.integers(8, 12)),
                num_y=count(14), num_cb=count(10), num_cr=count(10), points=_pick(rng, [("ends", 2), ("inner", 2), ("equal_y", 1)]),
                coeffs=_pick(rng, [("stable", 3), ("full", 1)]), csfl=bool(rng.random() < 0.3), overlap=bool(rng.random() < 0.65),
                mults=[int(_pick(rng, [(0, 1), (128, 2), (255, 1), (511 if i % 3 == 2 else 192, 1)])) for i in range(6)],
                seed=int(rng.integers(0, 1 << 16)) if seed == "uni" else int(seed), clip=bool(rng.random() < 0.3),
                mc_identity=bool(rng.random() < 0.5), kind=_pick(rng, [("noise", 4), ("zero", 1), ("max", 1), ("ramp", 1)]),
                sseed=int(rng.integers(0, 1 << 30)))


def segment_of(c: dict):
    """The grain table segment of a render case (its details drawn from the case's `sseed`)."""
    from grav1synth_amd.diff import GrainTableSegment

    rng = np.random.default_rng([c["sseed"], 1])
    lag = c["lag"]
    n = 2 * lag * (lag + 1)

    def coeffs(extra):
        if c["coeffs"] == "full":  # the whole int8 range: the filter diverges and the template clamps at both ends
            v = rng.integers(-128, 128, n + extra)
            if n:
                v[n - 1] = 127 if extra == 0 else -128
        else:
            v = rng.integers(-12, 13, n + extra)
            if n:
                v[n - 1] = 50
                v[n - 1 - (lag + 1)] = 30
            if extra:
                v[n] = int(rng.integers(-60, 61))
        return [int(x) for x in v]

    def points(k, lo, hi):
        if k == 0:
            return []
        if c["points"] == "inner" or k == 1:
            xs = sorted(rng.choice(np.arange(1, 255), size=k, replace=False).tolist())
        else:
            xs = [0] + sorted(rng.choice(np.arange(1, 255), size=k - 2, replace=False).tolist()) + [255]
        ys = [int(rng.integers(lo, hi)) for _ in xs]
        if c["points"] == "equal_y":  # equal neighbouring scaling values: a flat piece of the table
            ys = [ys[i - (i & 1)] for i in range(len(ys))]
        return [(int(x), y) for x, y in zip(xs, ys)]

    m = c["mults"]
    return GrainTableSegment(
        random_seed=c["seed"], start_time=0, end_time=2 ** 63 - 1, scaling_points_y=points(c["num_y"], 20, 256),
        scaling_points_cb=points(c["num_cb"], 0, 256), scaling_points_cr=points(c["num_cr"], 0, 120), scaling_shift=c["scaling_shift"],
        ar_coeff_lag=lag, ar_coeffs_y=coeffs(0), ar_coeffs_cb=coeffs(1), ar_coeffs_cr=coeffs(1), ar_coeff_shift=c["ar_shift"],
        cb_mult=m[0], cb_luma_mult=m[1], cb_offset=m[2], cr_mult=m[3], cr_luma_mult=m[4], cr_offset=m[5],
        chroma_scaling_from_luma=c["csfl"], grain_scale_shift=c["gss"], overlap_flag=c["overlap"])


def plane_shapes(w: int, h: int, ss: str, round_up=True):
    """[(rows, columns)] of the planes: chroma rounded up ((w + 1) >> 1) as render and denoise take it, or down."""
    if ss == "mono":
        return [(h, w)]
    sx, sy = SUBSAMPLINGS[ss]
    r = (sx, sy) if round_up else (0, 0)
    return [(h, w)] + [((h + r[1]) >> sy, (w + r[0]) >> sx)] * 2


def _fill(rng, shape, bd: int, kind: str, i: int = 0) -> np.ndarray:
    top = (1 << bd) - 1
    if kind == "noise":
        p = rng.integers(0, top + 1, shape)
    elif kind == "zero":
        p = np.zeros(shape, np.int64)
    elif kind in ("max", "const"):
        p = np.full(shape, top)
    elif kind == "ramp":
        p = (np.arange(shape[0] * shape[1]).reshape(shape) * (7 + i)) % (top + 1)
    elif kind == "flat":
        p = np.full(shape, (top * 5) // 16) + rng.integers(-(1 << (bd - 8)), (1 << (bd - 8)) + 1, shape)
    else:  # gradient with noise of a few 8-bit steps
        amp = 5 << (bd - 8)
        base = ((np.arange(shape[1])[None, :] * (3 + i) + np.arange(shape[0])[:, None] * (2 + i)) << (bd - 8)) % (top + 1)
        p = np.clip(base + rng.integers(-amp, amp + 1, shape), 0, top)
    return np.ascontiguousarray(np.clip(p, 0, top).astype(np.uint8 if bd == 8 else np.uint16))


def render_planes(c: dict):
    rng = np.random.default_rng([c["sseed"], 2])
    return [_fill(rng, s, c["bd"], c["kind"], i) for i, s in enumerate(plane_shapes(c["w"], c["h"], c["ss"]))]


# ---- denoise ------------------------------------------------------------------------------------------------------------

STRENGTHS = [(0.05, 1), (1.0, 1), (4.0, 2), (60.0, 1), (1000.0, 1)]
DN_KINDS = [("grainy", 3), ("gradient", 3), ("noise", 2), ("const", 1)]


def _dn(w, h, bd, ss, A, S, strength, chroma_strength, kind, **kw) -> dict:
    c = dict(w=w, h=h, wc=_cls(w, 64), hc=_cls(h, 48), pool=-1, bd=bd, ss=ss, A=A, S=S, strength=strength, chroma_strength=chroma_strength, kind=kind,
             cseed=w * 977 + h)
    c.update(kw)
    return c


_FORCED_DENOISE = [
    _dn(65, 49, 12, "422", 3, 4, 4.0, 1.0, "grainy"), _dn(63, 47, 8, "420", 7, 4, 60.0, 4.0, "gradient"), _dn(129, 5, 10, "444", 7, 1, 0.05, 60.0, "noise"),
    _dn(1, 1, 8, "420", 3, 2, 4.0, 4.0, "noise"), _dn(2, 97, 10, "422", 1, 4, 1.0, 1000.0, "grainy"), _dn(64, 48, 12, "mono", 7, 4, 1000.0, 1000.0, "const"),
    _dn(128, 96, 10, "420", 1, 1, 4.0, 0.05, "gradient"), _dn(66, 50, 8, "444", 2, 4, 4.0, 4.0, "grainy"), _dn(3, 7, 12, "420", 5, 3, 60.0, 0.05, "noise"),
]


def _dn_budget(c: dict, frames: int, window: int) -> float:
    """What the numpy reference pays for a case: samples x offsets x frames x neighbours."""
    px = sum(a * b for a, b in plane_shapes(c["w"], c["h"], c["ss"]))
    return px * (2 * c["A"] + 1) ** 2 * frames * window


POOL = 8  # parameter sets a list draws from: a Denoiser's parameters are fixed when it is made, and it is the same object
#           meeting another geometry that the sweep is after


def _dn_pool(rng, temporal: bool) -> List[dict]:
    """POOL parameter sets, stratified so that every entry of every menu is in the pool: a permutation of the menu, filled
    up with weighted draws."""
    def column(menu):
        vals = [m[0] for m in menu]
        col = [vals[i] for i in rng.permutation(len(vals))][:POOL]
        return col + [_pick(rng, menu) for _ in range(POOL - len(col))]

    A = column([(1, 2), (2, 1), (3, 2), (4, 1), (5, 1), (6, 1), (7, 2)])
    S_ = column([(1, 2), (2, 2), (3, 1), (4, 2)])
    h, hc, bd = column(STRENGTHS), column(STRENGTHS), column([(8, 1), (10, 1), (12, 1)])
    D, batch = column([(0, 1), (1, 2), (2, 2), (3, 2)]), column([(1, 1), (2, 1), (3, 1), (4, 1), (5, 1)])
    out = []
    for i in range(POOL):
        p = dict(bd=int(bd[i]), A=int(A[i]), S=int(S_[i]), strength=float(h[i]), chroma_strength=float(hc[i]))
        if temporal:
            p.update(D=int(D[i]), batch=int(batch[i]))
        out.append(p)
    return out


def _draw_dn_common(rng, pool) -> dict:
    w, wc = _edge(rng, 64, 3, (4, 200))
    h, hc = _edge(rng, 48, 3, (4, 150))
    k = int(rng.integers(0, len(pool)))
    p = pool[k]
    return dict(w=w, h=h, wc=wc, hc=hc, pool=k, bd=p["bd"], ss=_pick(rng, [("420", 3), ("422", 2), ("444", 2), ("mono", 1)]),
                A=p["A"], S=p["S"], strength=p["strength"], chroma_strength=p["chroma_strength"], kind=_pick(rng, DN_KINDS),
                cseed=int(rng.integers(0, 1 << 30)))


def _draw_denoise(rng, pool=None) -> dict:
    while True:  # (a case the reference would take seconds for is drawn again: the sizes stay small, the menus whole)
        c = _draw_dn_common(rng, pool)
        if _dn_budget(c, 1, 1) <= 6e6:
            return c


def _dnt(w, h, bd, ss, A, S, D, n, batch, nc, strength=4.0, chroma_strength=4.0, kind="grainy", split=-1, split_kind="none") -> dict:
    return dict(w=w, h=h, wc=_cls(w, 64), hc=_cls(h, 48), pool=-1, bd=bd, ss=ss, A=A, S=S, strength=strength, chroma_strength=chroma_strength, kind=kind,
                cseed=w * 977 + h + D, D=D, nframes=n, nc=nc, batch=batch, split=split, split_kind=split_kind)


_FORCED_DENOISE_T = [
    _dnt(40, 30, 12, "mono", 7, 1, 3, 7, 3, "2D+1", 1000.0, 1000.0, "const"),   # all-max, every weight 4096: the numerator past 2^32
    _dnt(65, 49, 12, "422", 2, 4, 2, 5, 2, "2D+1"), _dnt(63, 48, 8, "420", 3, 2, 3, 2, 1, "b+1"), _dnt(64, 47, 10, "444", 1, 1, 1, 4, 5, "2D+2", 60.0, 1.0, "noise"),
    _dnt(33, 25, 10, "420", 7, 2, 1, 3, 2, "2D+1", 0.05, 4.0, "gradient", split=2, split_kind="geometry"),
    _dnt(70, 20, 8, "422", 2, 2, 3, 8, 4, "2D+2", split=4, split_kind="sync"), _dnt(1, 1, 8, "420", 3, 2, 2, 3, 2, "D+1"),
    _dnt(3, 50, 10, "444", 4, 3, 0, 4, 3, "b+1"),
]


def _draw_denoise_t(rng, pool=None) -> dict:
    while True:
        c = _draw_dn_common(rng, pool)
        p = pool[c["pool"]]
        D, batch = p["D"], p["batch"]
        nc = _pick(rng, [("1", 1), ("D", 1.5), ("D+1", 1.5), ("2D", 1.5), ("2D+1", 1.5), ("2D+2", 1.5), ("b-1", 1), ("b+1", 1)])
        n = max({"1": 1, "D": D, "D+1": D + 1, "2D": 2 * D, "2D+1": 2 * D + 1, "2D+2": 2 * D + 2, "b-1": batch - 1, "b+1": batch + 1}[nc], 1)
        split, split_kind = -1, "none"
        if n >= 2:
            split_kind = _pick(rng, [("none", 3), ("sync", 1), ("geometry", 1)])
            if split_kind != "none":
                split = int(rng.integers(1, n))
        c.update(D=D, nframes=n, nc=nc, batch=batch, split=split, split_kind=split_kind)
        if _dn_budget(c, n, min(2 * D + 1, n)) <= 2.5e7:
            return c


def denoise_frames(c: dict, n: int = 1):
    """n frames of a denoise case: grain on a window that moves over a larger picture, noisy gradients, full-range noise or
    a constant (the maximum)."""
    from tests.content import make_frames

    rng = np.random.default_rng([c["cseed"], 3])
    shapes = plane_shapes(c["w"], c["h"], c["ss"])
    bd, top = c["bd"], (1 << c["bd"]) - 1
    frames = []
    if c["kind"] == "grainy":
        sx, sy = SUBSAMPLINGS["420" if c["ss"] == "mono" else c["ss"]]
        big = make_frames("distinct", c["w"] + 64, c["h"] + 64, bd, sx, sy, frame=c["cseed"] & 7)[1]
    for t in range(n):
        planes = []
        for i, s in enumerate(shapes):
            if c["kind"] == "grainy":
                ox, oy = (3 * t) % 30, ((t * t) // 2) % 30
                amp = (3 + 2 * i) << (bd - 8)
                p = big[i][oy:oy + s[0], ox:ox + s[1]].astype(np.int64) + rng.integers(-amp, amp + 1, s)
                planes.append(np.ascontiguousarray(np.clip(p, 0, top).astype(np.uint8 if bd == 8 else np.uint16)))
            else:
                planes.append(_fill(rng, s, bd, c["kind"], i))
        frames.append(planes)
    return frames


def other_geometry(c: dict):
    """The frame that interrupts a clip when `split_kind` is "geometry": another size and subsampling."""
    o = dict(c, w=c["w"] + 3, h=c["h"] + 1, ss="444" if c["ss"] != "444" else "420", kind="gradient", cseed=c["cseed"] + 1)
    return o, denoise_frames(o, 1)[0]


# ---- estimate -----------------------------------------------------------------------------------------------------------

# k_estimate[_pk]: a wave owns 496 output columns (8 a lane, lanes 0 and 63 the halo words) of a strip of rows -- 32 rows, or for the
# packed kernel 8 .. 256 rows chosen from the device's occupancy; the second column strip begins at W - 1 > 496.  (At the sizes
# drawn here the packed kernel's choice is 8 rows; its other heights, pinned: tests/test_gpu_estimate_strips.py.)
EST_COLS, EST_ROWS = 496, 32


def _est(w, h, bd, kind, where) -> dict:
    return dict(w=w, h=h, wc=_cls(w, EST_COLS, True), hc=_cls(h, EST_ROWS, True), bd=bd, kind=kind, where=where, cseed=w * 7 + h)


_FORCED_ESTIMATE = [
    _est(1, 1, 8, "noise", "device"), _est(2, 50, 10, "flat", "device"), _est(3, 3, 12, "flat", "strided"), _est(50, 2, 8, "flat", "host"),
    _est(1, 40, 10, "flat", "device"), _est(495, 5, 8, "gradient", "device"), _est(496, 34, 10, "flat", "strided"), _est(497, 3, 12, "gradient", "device"),
    _est(498, 9, 8, "flat", "host"), _est(499, 33, 10, "gradient", "strided"), _est(991, 4, 8, "flat", "device"), _est(992, 35, 12, "gradient", "strided"),
    _est(993, 7, 10, "flat", "device"), _est(1489, 3, 8, "gradient", "device"),
]


def _draw_estimate(rng) -> dict:
    w, wc = _edge(rng, EST_COLS, 2, (4, 300), plus2=True)
    h, hc = _edge(rng, EST_ROWS, 9, (4, 200), plus2=True)
    return dict(w=w, h=h, wc=wc, hc=hc, bd=int(_pick(rng, [(8, 1), (10, 1), (12, 1)])), kind=_pick(rng, [("gradient", 3), ("flat", 2), ("noise", 2), ("synth", 2)]),
                where=_pick(rng, [("device", 2), ("strided", 2), ("host", 1)]), cseed=int(rng.integers(0, 1 << 30)))


def estimate_plane(c: dict) -> np.ndarray:
    if c["kind"] == "synth":
        from grav1synth_amd.synth import SynthSpec, make_pair

        return make_pair(SynthSpec(c["w"], c["h"], c["bd"], nplanes=1), c["cseed"] & 15)[0][0].numpy()
    return _fill(np.random.default_rng([c["cseed"], 4]), (c["h"], c["w"]), c["bd"], c["kind"])


# ---- resize -------------------------------------------------------------------------------------------------------------

_FORCED_RESIZE = [
    dict(alg=a, w=w, h=h, tw=tw, th=th, sc="odd", twc=twc, thc=thc, bd=bd, ss=ss, where="device", cseed=k)
    for k, (a, w, h, tw, th, twc, thc, bd, ss) in enumerate([
        ("lanczos", 128, 64, 16, 128, "/8", "x2", 8, "420"), ("hermite", 129, 33, 16, 8, "/8", "/8+1", 10, "444"),
        ("spline36", 96, 80, 12, 10, "/8", "/8", 12, "420"), ("catmullrom", 160, 48, 20, 96, "/8", "x2", 10, "422"),
        ("mitchell", 64, 160, 128, 20, "x2", "/8", 8, "444")])
]


def _draw_resize(rng) -> dict:
    ss = _pick(rng, [("420", 3), ("422", 1), ("444", 2)])
    sx, sy = SUBSAMPLINGS[ss]

    def src(cap):
        c = _pick(rng, [("2", 0.5), ("3", 0.5), ("odd", 3), ("even", 3), ("m16", 2)])
        return {"2": 2, "3": 3, "odd": 2 * int(rng.integers(2, cap // 2)) + 1, "even": 2 * int(rng.integers(2, cap // 2)),
                "m16": 16 * int(rng.integers(1, cap // 16 + 1))}[c], c

    def dst(s, sub):
        c = _pick(rng, [("2", 1), ("3", 1), ("odd", 2), ("x2", 2), ("/2", 2), ("/8", 1.5), ("/8+1", 1.5), ("same", 1.5)])
        v = {"2": 2, "3": 3, "odd": 2 * int(rng.integers(1, 100)) + 1, "x2": 2 * s, "/2": s // 2, "/8": s // 8, "/8+1": s // 8 + 1, "same": s}[c]
        v = max(v, 1 << sub)
        return (v + ((1 << sub) - 1)) & ~((1 << sub) - 1), c  # (a target is a multiple of the chroma subsampling)

    w, wsc = src(200)
    h, hsc = src(150)
    if w < 2 << sx or h < 2 << sy:  # (a chroma plane of at least two samples)
        w, h, wsc, hsc = max(w, 2 << sx), max(h, 2 << sy), "min" if w < 2 << sx else wsc, "min" if h < 2 << sy else hsc
    tw, twc = dst(w, sx)
    th, thc = dst(h, sy)
    return dict(alg=str(_pick(rng, [(a, 1) for a in ALGS])), w=w, h=h, tw=tw, th=th, sc=wsc + "," + hsc, twc=twc, thc=thc,
                bd=int(_pick(rng, [(8, 1), (10, 1), (12, 1)])), ss=ss, where=_pick(rng, [("device", 1), ("host", 1)]), cseed=int(rng.integers(0, 1 << 30)))


def resize_planes_of(c: dict):
    """Full-range noise with a saturated band and an empty patch (the clamp); chroma planes are (w >> xdec, h >> ydec)."""
    rng = np.random.default_rng([c["cseed"], 5])
    planes = [_fill(rng, s, c["bd"], "noise") for s in plane_shapes(c["w"], c["h"], c["ss"], round_up=False)]
    h, w = planes[0].shape
    planes[0][: h // 4] = (1 << c["bd"]) - 1
    planes[0][h // 4: h // 2, : w // 3] = 0
    return planes
