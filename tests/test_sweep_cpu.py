"""tests/sweep.py is what it says, without a device: the lists are deterministic and pasteable, the committed (seed, n) of
every operation draws every entry of every menu (so that shrinking a list or editing a menu cannot drop an edge unseen), and
the references agree with each other where a drawn case has two."""
from __future__ import annotations

import numpy as np
import pytest

from tests import sweep as S


def _have(cases, field):
    return {c[field] for c in cases}


def _need(cases, field, wanted, what):
    missing = set(wanted) - _have(cases, field)
    assert not missing, f"{cases[0]['op']}: no case draws {what} {sorted(map(str, missing))} (field {field!r})"


@pytest.mark.parametrize("op", S.OPS)
def test_lists_are_deterministic_seeded_and_pasteable(op):
    seed, n, chunks = S.SUITE[op]
    a, b = S.cases(op, seed, n), S.cases(op, seed, n)
    assert a == b and S.digest(a) == S.digest(b)
    assert S.cases(op, seed + 1, n) != a, "another seed, another list"
    assert S.cases(op, seed, n + 5)[:n] == a, "a longer list goes on from the shorter one"
    for c in a:
        assert eval(repr(c)) == c, c
        assert all(isinstance(v, (int, float, str, bool, list)) for v in c.values()), c
    parts = [S.chunk_of(a, k, chunks) for k in range(chunks)]
    assert sorted(c["i"] for p in parts for c in p) == list(range(n)) and all(parts), "the chunks share out every case once"
    assert any(c["forced"] for p in parts for c in p[:2])
    with pytest.raises(ValueError):
        S.cases("sharpen", 1, 1)


def test_diff_list_covers_its_menus():
    cs = S.suite_cases("diff")
    _need(cs, "wc", ["32k-1", "32k", "32k+1", "128k", "128k+16", "128k-16", "16m", "16m+8", "16m+1", "16m-1", "uni", "blocks"], "the width class")
    _need(cs, "hc", ["32k-1", "32k", "32k+1", "uni"], "the height class")
    _need(cs, "blocks", [1023, 1024, 1025, 2047, 2048, 4095, 4096, 4097], "the block count")
    _need(cs, "lag", [1, 2, 3], "lag")
    _need(cs, "ss", ["420", "422", "444"], "subsampling")
    _need(cs, "chroma", [True, False], "chroma / luma-only")
    _need(cs, "batch", [1, 2, 3, 4, 5], "batch_frames")
    _need(cs, "nc", ["kb-1", "kb", "kb+1", "ring"], "the frame count class")
    _need(cs, "cutc", ["none", "edge", "inside"], "a scene cut on / off a batch edge")
    _need(cs, "k3", ["", "stream"], "the accumulation chain")
    _need(cs, "latest", ["", "host", "device"], "the half of the fold")
    _need(cs, "where", ["host", "device"], "the frames' memory")
    _need(cs, "content", ["synth", "content"], "the content family")
    pairs = {(c["src_bd"], c["den_bd"]) for c in cs}
    assert {(8, 8), (10, 10), (12, 12)} <= pairs and any(a != b for a, b in pairs), "equal and mixed depth pairs"
    assert {"distinct", "flat", "busy", "damaged", "clamped"} <= {k for c in cs for k in c["kinds"]}
    # the wide chain: rows of whole 8-sample words in every plane, luma a whole number of 128-sample units or not
    wide = [c for c in cs if c["w"] % 8 == 0 and (c["w"] >> S.SUBSAMPLINGS[c["ss"]][0]) % 8 == 0 and c["blocks"] < 1000]
    assert any(c["w"] % 128 == 0 for c in wide) and any(c["w"] % 128 == 16 << S.SUBSAMPLINGS[c["ss"]][0] for c in wide) and len(wide) >= 8
    assert any(c["k3"] == "stream" for c in wide), "G1S_K3=stream at a geometry the wide chain would serve"
    assert any(c["nframes"] > S.KSLOTS * c["batch"] for c in cs), "more batches than slots: the ring goes round"
    assert any(c["cut"] > 0 and c["cut"] % c["batch"] == 0 and c["batch"] > 1 for c in cs), "a cut on the edge of a batch of several frames"
    assert any(c["latest"] == "" and c["blocks"] >= 4096 for c in cs) and any(c["latest"] == "" and c["blocks"] == 4095 for c in cs)
    assert any(c["latest"] == "device" and c["blocks"] in (1025, 2047) for c in cs), "k4_latest with a short last chunk"
    # (from 1 000 blocks the device half's latest states are compared with the host half's: tests/test_gpu_sweep._latest_mismatches)
    assert any(c["blocks"] > 1024 and c["textured"] for c in cs) and any(c["blocks"] > 1024 and not c["textured"] for c in cs), "chunks of one bin and of several"
    for c in cs:
        assert 1 <= c["nframes"] and len(c["kinds"]) in (0, c["nframes"]) and c["cut"] < c["nframes"] and min(c["w"], c["h"]) >= 66


def test_render_list_covers_its_menus():
    from tests import grain_ref as R

    cs = S.suite_cases("render")
    _need(cs, "wc", ["1", "2", "3", "ku-1", "ku", "ku+1", "ku+2", "uni"], "the width class")
    _need(cs, "hc", ["ku-1", "ku", "ku+1", "ku+2", "uni"], "the height class")
    for f, vals in (("bd", [8, 10, 12]), ("ss", ["420", "422", "444", "mono"]), ("lag", [0, 1, 2, 3]), ("ar_shift", [6, 7, 8, 9]),
                    ("gss", [0, 1, 2, 3]), ("scaling_shift", [8, 9, 10, 11]), ("num_y", [0, 1, 2, 10, 14]), ("num_cb", [0, 1, 2, 10]),
                    ("num_cr", [0, 1, 2, 10]), ("points", ["ends", "inner", "equal_y"]), ("coeffs", ["stable", "full"]), ("csfl", [True, False]),
                    ("overlap", [True, False]), ("clip", [True, False]), ("kind", ["noise", "zero", "max", "ramp"])):
        _need(cs, f, vals, f)
    assert {0, 1, 0x8000, 0xFFFF} <= _have(cs, "seed") and any(c["seed"] not in (0, 1, 0x8000, 0xFFFF) for c in cs)
    assert {0, 128, 255} <= {m for c in cs for m in c["mults"]} and any(511 in (c["mults"][2], c["mults"][5]) for c in cs)
    assert {(True, True), (True, False)} <= {(c["clip"], c["mc_identity"]) for c in cs}, "restricted range with and without an identity matrix"
    # a last block of one and of two columns / rows with the overlap blend on, in the subsampled and the full-size planes
    for ss in ("420", "444"):
        for rem in (1, 2):
            assert any(c["overlap"] and c["ss"] == ss and c["w"] > 32 and c["w"] % 32 == rem for c in cs), f"overlap, {ss}, a last block of {rem} columns"
            assert any(c["overlap"] and c["ss"] == ss and c["h"] > 32 and c["h"] % 32 == rem for c in cs), f"overlap, {ss}, a last stripe of {rem} rows"
    assert any(c["ss"] in ("420", "422") and c["w"] % 2 for c in cs), "an odd width with subsampled chroma"
    # full-range coefficients make the template clamp at both ends of the grain range
    full = [c for c in cs if c["coeffs"] == "full" and c["lag"] >= 2 and c["num_y"] > 0][:2]
    assert full
    for c in full:
        luma = R.generate_grain(S.segment_of(c), c["bd"], 0, 0, mono=True)[0]
        assert (luma.min(), luma.max()) == R.grain_range(c["bd"]), f"case {c['i']}: the template saturates at both ends"
    for c in cs:
        seg = S.segment_of(c)
        for pts, cap in ((seg.scaling_points_y, 14), (seg.scaling_points_cb, 10), (seg.scaling_points_cr, 10)):
            xs = [p[0] for p in pts]
            assert len(pts) <= cap and xs == sorted(set(xs)) and all(0 <= v <= 255 for p in pts for v in p), c
        assert all(-128 <= v <= 127 for v in seg.ar_coeffs_y + seg.ar_coeffs_cb + seg.ar_coeffs_cr)
    ends = [S.segment_of(c) for c in cs if c["points"] == "ends" and c["num_y"] >= 2]
    assert ends and all(s.scaling_points_y[0][0] == 0 and s.scaling_points_y[-1][0] == 255 for s in ends)
    eq = [S.segment_of(c) for c in cs if c["points"] == "equal_y" and c["num_y"] >= 2]
    assert eq and all(s.scaling_points_y[0][1] == s.scaling_points_y[1][1] for s in eq)


def _denoise_common(cs):
    _need(cs, "wc", ["ku-1", "ku", "ku+1", "uni", "1", "2", "3"], "the width class")
    _need(cs, "hc", ["ku-1", "ku", "ku+1", "uni"], "the height class")
    for f, vals in (("bd", [8, 10, 12]), ("ss", ["420", "422", "444", "mono"]), ("A", [1, 2, 3, 4, 5, 6, 7]), ("S", [1, 2, 3, 4]),
                    ("strength", [0.05, 1.0, 4.0, 60.0, 1000.0]), ("chroma_strength", [0.05, 1.0, 4.0, 60.0, 1000.0]),
                    ("kind", ["grainy", "gradient", "noise", "const"])):
        _need(cs, f, vals, f)
    assert any(c["strength"] != c["chroma_strength"] for c in cs)
    assert any(c["A"] == 7 and c["S"] == 4 for c in cs) and any(c["S"] == 4 and c["w"] % 64 == 1 and c["ss"] == "422" and c["bd"] == 12 for c in cs)
    assert any(c["ss"] in ("420", "422") and c["w"] % 2 for c in cs), "an odd width with subsampled chroma"


def test_denoise_lists_cover_their_menus():
    from grav1synth_amd.denoise import weight_table

    cs = S.suite_cases("denoise")
    _denoise_common(cs)
    assert weight_table(8, 2, 0.05)[1] == 0 and weight_table(12, 1, 1000.0)[1] >= 10, "the strengths reach q = 0 and a large q"
    ct = S.suite_cases("denoise_t")
    _denoise_common(ct)
    _need(ct, "D", [0, 1, 2, 3], "the temporal radius")
    _need(ct, "nc", ["1", "D", "D+1", "2D", "2D+1", "2D+2", "b-1", "b+1"], "the clip length class")
    _need(ct, "batch", [1, 2, 3, 4, 5], "batch_frames")
    _need(ct, "split_kind", ["none", "sync", "geometry"], "what ends a clip early")
    assert any(c["nframes"] <= c["D"] for c in ct), "a clip shorter than the window's half"
    assert any(c["nframes"] == 2 * c["D"] + 1 and c["D"] == 3 for c in ct) and any(c["nframes"] > 2 * c["D"] + 1 and c["D"] >= 1 for c in ct)
    assert any(c["nframes"] > c["batch"] > 1 and c["D"] >= 1 for c in ct), "a window across a batch edge"
    big = [c for c in ct if c["kind"] == "const" and c["bd"] == 12 and c["strength"] == 1000.0
           and (2 * c["A"] + 1) ** 2 * min(2 * c["D"] + 1, c["nframes"]) * 4096 * 4095 >= 2 ** 32]
    assert big, "all-max at 12 bits with every weight 4096: a numerator beyond 32 bits"
    # a Denoiser's parameters are fixed when it is made: the lists draw them from a pool, so that inside a chunk the same
    # object meets another geometry (tests/test_gpu_sweep.py keeps it by these keys)
    for op, cases, least in (("denoise", cs, 30), ("denoise_t", ct, 10)):
        chunks, again = S.SUITE[op][2], 0
        for k in range(chunks):
            seen = {}
            for c in S.chunk_of(cases, k, chunks):
                key = (c["bd"], c["A"], c["S"], c["strength"], c["chroma_strength"], c.get("D"), c.get("batch"))
                again += key in seen and seen[key] != (c["w"], c["h"], c["ss"])
                seen[key] = (c["w"], c["h"], c["ss"])
        assert again >= least, f"{op}: a kept Denoiser meets another geometry {again} times, {least} wanted"
    for c in ct:
        assert 1 <= c["nframes"] and (c["split"] == -1) == (c["split_kind"] == "none") and c["split"] < c["nframes"]


def test_estimate_and_resize_lists_cover_their_menus():
    cs = S.suite_cases("estimate")
    _need(cs, "wc", ["1", "2", "3", "ku-1", "ku", "ku+1", "uni"], "the width class")
    _need(cs, "hc", ["1", "2", "3", "ku-1", "ku", "ku+1", "uni"], "the height class")
    for f, vals in (("bd", [8, 10, 12]), ("kind", ["gradient", "flat", "noise", "synth"]), ("where", ["device", "strided", "host"])):
        _need(cs, f, vals, f)
    assert (1, 1) in {(c["w"], c["h"]) for c in cs} and any(c["w"] == 1 and c["h"] >= 3 for c in cs), "one sample wide, three rows or more"
    # the kernel's units: column strips of 496 output columns (the second begins at W - 1 > 496), row strips of 32 rows
    assert {495, 496, 497, 498, 499, 991, 992, 993} <= _have(cs, "w"), "widths round the first and the second column strip's end"
    assert sum(c["w"] - 1 > S.EST_COLS for c in cs) >= 8 and any(c["w"] - 1 > 2 * S.EST_COLS for c in cs), "a second and a third column strip"
    _need(cs, "hc", ["ku-1", "ku", "ku+1", "ku+2"], "a height round a multiple of the 32-row strip")
    assert any(c["w"] - 1 > S.EST_COLS and c["where"] == "strided" for c in cs), "a second column strip in a pitched view"
    cr = S.suite_cases("resize")
    for f, vals in (("alg", S.ALGS), ("bd", [8, 10, 12]), ("ss", ["420", "422", "444"]), ("where", ["device", "host"]),
                    ("twc", ["2", "3", "odd", "x2", "/2", "/8", "/8+1", "same"]), ("thc", ["2", "3", "odd", "x2", "/2", "/8", "/8+1", "same"])):
        _need(cr, f, vals, f)
    assert {2, 3} <= {c["tw"] for c in cr} | {c["th"] for c in cr} and {2, 3} <= {c["w"] for c in cr} | {c["h"] for c in cr}
    assert any(c["tw"] > c["w"] and c["th"] < c["h"] for c in cr) and any(c["tw"] < c["w"] and c["th"] > c["h"] for c in cr), "up in one axis, down in the other"
    assert any(c["ss"] == "420" and c["w"] % 2 and c["h"] % 2 for c in cr), "odd 4:2:0 sizes"
    for alg in S.ALGS:  # every algorithm takes a down-scale by 8 or more, where the window mirrors furthest
        assert any(c["alg"] == alg and (c["tw"] * 8 <= c["w"] or c["th"] * 8 <= c["h"]) for c in cr), alg
    for c in cr:
        sx, sy = S.SUBSAMPLINGS[c["ss"]]
        assert c["tw"] % (1 << sx) == 0 and c["th"] % (1 << sy) == 0 and c["tw"] >= 1 << sx and c["th"] >= 1 << sy, c
        assert all(min(p.shape) >= 1 for p in S.resize_planes_of(c))


def test_inputs_are_deterministic_and_of_the_declared_shape():
    for c in S.suite_cases("render")[:20]:
        a, b = S.render_planes(c), S.render_planes(c)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and S.segment_of(c) == S.segment_of(c)
        assert [p.shape for p in a] == S.plane_shapes(c["w"], c["h"], c["ss"]) and a[0].dtype == (np.uint8 if c["bd"] == 8 else np.uint16)
        if c["ss"] in ("420", "422"):
            assert a[1].shape[1] == (c["w"] + 1) >> 1
    for c in S.suite_cases("denoise_t")[:12]:
        fr = S.denoise_frames(c, c["nframes"])
        assert len(fr) == c["nframes"] and all(np.array_equal(x, y) for f, g in zip(fr, S.denoise_frames(c, c["nframes"])) for x, y in zip(f, g))
        if c["kind"] == "const":
            assert all((p == (1 << c["bd"]) - 1).all() for f in fr for p in f)
        elif c["nframes"] > 1 and c["w"] * c["h"] > 16:
            assert (fr[0][0] != fr[1][0]).any(), "the frames of a clip differ"
    for c in [c for c in S.suite_cases("diff") if c["blocks"] < 100][:6]:
        fr = S.diff_frames(c)
        assert len(fr) == c["nframes"] and len(fr[0][0]) == (3 if c["chroma"] else 1) and fr[0][0][0].shape == (c["h"], c["w"])
        assert fr[0][0][0].dtype == (np.uint8 if c["src_bd"] == 8 else np.uint16) and fr[0][1][0].dtype == (np.uint8 if c["den_bd"] == 8 else np.uint16)


def test_the_two_denoise_references_agree_on_the_smallest_drawn_cases():
    """The vectorised references against the rules written out as loops (test_denoise_cpu / test_denoise_temporal_cpu)."""
    from grav1synth_amd.denoise import weight_table
    from tests import denoise_ref as R
    from tests import denoise_temporal_ref as TR
    from tests.test_denoise_cpu import direct
    from tests.test_denoise_temporal_cpu import direct as direct_t

    def cost(c):
        return c["w"] * c["h"] * (2 * c["A"] + 1) ** 2 * (2 * c["S"] + 1) ** 2 * c.get("nframes", 1) * (2 * c.get("D", 0) + 1)

    small = sorted((c for c in S.suite_cases("denoise") if cost(c) <= 4e5), key=cost)[:3]
    assert small
    for c in small:
        u = S.denoise_frames(c, 1)[0][0]
        T, q = weight_table(c["bd"], c["S"], c["strength"])
        assert np.array_equal(R.denoise_plane(u, c["A"], c["S"], T, q), direct(u, c["A"], c["S"], T, q)), c
    small = sorted((c for c in S.suite_cases("denoise_t") if cost(c) <= 4e5), key=cost)[:3]
    assert small
    for c in small:
        planes = [f[0] for f in S.denoise_frames(c, c["nframes"])]
        T, q = weight_table(c["bd"], c["S"], c["strength"])
        got = TR.denoise_plane_clip(planes, c["D"], c["A"], c["S"], T, q)
        for t in range(len(planes)):
            assert np.array_equal(got[t], direct_t(planes, t, c["D"], c["A"], c["S"], T, q)), (c, t)
