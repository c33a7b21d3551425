"""tests/test_gpu_int8_edges.py feeds what it means to, without a device: from the ORACLE's masks and shadows of its jobs, the
residuals recomputed from the planes, and a restatement of the launch arithmetic (engine.hip w_wgs_per_frame / m_wgs_per_frame,
the kernels' own cut of a list into slices).

  * the oracle accepts every frame (the jobs raise otherwise) and finds every block flat;
  * -129, -128, 127 and 128 occur in the narrowed residual exactly where a design put them, and the field around them is benign;
  * the luma sums under the chroma samples hit 127 / 128 / -128 / -129 exactly where designed and stay small elsewhere, with every
    member inside int8 (4:4:4 apart, where L is the residual);
  * the poked units are, under the workgroups a frame of the cases, a ghost in front of a slice, a ghost behind one, the last unit
    of an odd slice and a slice's interior;
  * the bound cases' lists have the designed length, their longest slice is the cap (100, 32; the stream chain's reaches 0.9 of
    kMMaxUnits - 16 and never exceeds kMMaxUnits), the middle slice has a ghost at both ends, the largest luma S entry exceeds
    2^32 and the bound of a wave's accumulator over the longest slice exceeds 2^30;
  * each kind of case bites: against a reference that wrapped the poked residual, or L, to int8, or reduced S mod 2^32,
    record_mismatches names the fields.

These are conditions on the content, not measurements: a geometry that misses one is changed, not the condition."""
import numpy as np
import pytest

from tests import int8_content as IC
from tests.helpers import record_mismatches
from tests.test_gpu_int8_edges import BOUNDS, GEOMS, UNIT_W, VALUES, WGS, _bound_job, _job, _run_oracle, _whole_units, plane_dims, residuals
from tests.test_gpu_k3w_slices import slices, unit_list

K_W_MAX_UNITS, K_W_MAX_UNITS_C, K_M_MAX_UNITS = 100, 32, 240  # k3w.hip.h kWMaxUnits, kWMaxUnitsC; k3m.hip.h kMMaxUnits


# ---- the launch arithmetic, restated --------------------------------------------------------------------------------------------

def w_wgs_per_frame(ncell: int, kind: int, v: int) -> int:
    """engine.hip w_wgs_per_frame with G1S_W_WGS[_C] = v in 1 .. 7: that many workgroups a frame, but never fewer than the cap asks."""
    assert 1 <= v < 8
    cap = K_W_MAX_UNITS_C if kind else K_W_MAX_UNITS
    return max(-(-ncell // cap), v)


def m_wgs_per_frame(nunits: int, batch: int, f_wgs: int) -> int:
    """engine.hip m_wgs_per_frame with G1S_F_WGS = f_wgs."""
    gmin = -(-nunits // (K_M_MAX_UNITS - 16))
    target = max(8, f_wgs)
    return (max(gmin, -(-target // max(batch, 1))) + 7) & ~7


def stream_lists(flat: np.ndarray, geom):
    """(general units, plain units) of a frame as k3m_units counts them: a unit is two blocks of a block row with a flat block; it is
    plain when both are flat and the window of each is the whole block, in the luma and in the chroma planes."""
    nbh, nbw = flat.shape
    kinds = [(32, 32, geom.w, geom.h)]
    if geom.chroma:
        kinds.append((32 >> geom.xd, 32 >> geom.yd, geom.w >> geom.xd, geom.h >> geom.yd))
    at = lambda x, y: bool(flat[y, x]) if 0 <= x < nbw and 0 <= y < nbh else False
    n_general = n_plain = 0
    for by in range(nbh):
        for ci in range(-(-nbw // 2)):
            bits = [at(2 * ci + b, by) for b in (0, 1)]
            if not any(bits):
                continue
            plain = all(bits)
            for b in (0, 1):
                if not bits[b]:
                    continue
                bx = 2 * ci + b
                for bw, bh, pw, ph in kinds:
                    ys, xs = (0 if at(bx, by - 1) else geom.lag), (0 if at(bx - 1, by) else geom.lag)
                    ye, xe = min(ph - by * bh, bh), min(pw - bx * bw - geom.lag, bw if at(bx + 1, by) else bw - geom.lag)
                    if not (xe > xs and ye > ys) or (xs, ys, xe, ye) != (0, 0, bw, bh):
                        plain = False
            n_plain += plain
            n_general += not plain
    return n_general, n_plain


def stream_slices(n_general: int, n_plain: int, wgs: int):
    """Units of every workgroup: k3s_fused's `share` of the plain and of the general list, each with its own rounding."""
    share = lambda cnt, j: cnt * (j + 1) // wgs - cnt * j // wgs
    return [share(n_plain, j) + share(n_general, j) for j in range(wgs)]


# ---- A, B, C ---------------------------------------------------------------------------------------------------------------------

def _flat(shadow):
    return shadow["mask"] != 0


@pytest.mark.parametrize("name", list(GEOMS))
def test_every_block_of_every_frame_is_flat(name):
    sps, frames, shadows = _job(name)
    assert len(sps) == len(frames) == len(shadows)
    for sp, sh in zip(sps, shadows):
        assert _flat(sh).all(), f"{name}, {sp.label}: {int((~_flat(sh)).sum())} blocks not flat"
        assert all(ar[2] > 0 for ar in sh["ar"]), f"{name}, {sp.label}: a plane without observations"


@pytest.mark.parametrize("name", list(GEOMS))
def test_the_edge_values_lie_where_designed_and_nowhere_else(name):
    geom = GEOMS[name][0]
    sps, frames, _ = _job(name)
    seen = {(c, v): 0 for c in range(3 if geom.chroma else 1) for v in VALUES}
    for k, (sp, (s, d)) in enumerate(zip(sps, frames)):
        got = IC.narrowed_residuals(s, d, geom.src_bd, geom.den_bd)
        want = residuals(geom, k, sp)
        for c, (g_, w_) in enumerate(zip(got, want)):
            assert np.array_equal(g_, w_), f"{name}, {sp.label}: plane {c}'s residual is not the design"
            if sp.section == "C":
                assert np.isin(g_, (-128, 127)).all() or sp.fields[c] == "benign", f"{name}, {sp.label}: plane {c}"
                continue
            designed = {}
            for pc, y, x, v in sp.pokes:
                if pc == c:
                    designed[(y, x)] = v
            if c == 0 and (1 << geom.xd) * (1 << geom.yd) == 1:
                for cy, cx, v in sp.lsets:
                    designed[(cy, cx)] = v
            for v in VALUES:
                at = {(int(y), int(x)) for y, x in np.argwhere(g_ == v)}
                assert at == {p for p, pv in designed.items() if pv == v}, f"{name}, {sp.label}: plane {c}, {v} at {sorted(at)[:6]}"
                seen[(c, v)] += len(at)
            rest = np.ones(g_.shape, bool)
            for (y, x) in designed:
                rest[y, x] = False
            if c == 0:
                for cy, cx, _ in sp.lsets:
                    rest[cy << geom.yd:(cy + 1) << geom.yd, cx << geom.xd:(cx + 1) << geom.xd] = False
            assert np.abs(g_[rest]).max() <= 3, f"{name}, {sp.label}: plane {c} is not benign around the design"
    assert all(n > 0 for n in seen.values()), f"{name}: a value no frame holds: {seen}"


@pytest.mark.parametrize("name", [n for n, (g, _) in GEOMS.items() if g.chroma])
def test_the_luma_sums_hit_the_edge_exactly_where_designed(name):
    geom = GEOMS[name][0]
    sps, frames, _ = _job(name)
    members = (1 << geom.xd) * (1 << geom.yd)
    hit = set()
    for sp, (s, d) in zip(sps, frames):
        if sp.section != "B":
            continue
        res = IC.narrowed_residuals(s, d, geom.src_bd, geom.den_bd)[0]
        L = IC.luma_sums(res, geom.xd, geom.yd)
        assert L.shape == s[1].shape
        want = {(cy, cx): v for cy, cx, v in sp.lsets}
        assert len(want) >= 3
        for v in VALUES:
            at = {(int(y), int(x)) for y, x in np.argwhere(L == v)}
            assert at == {p for p, pv in want.items() if pv == v}, f"{name}, {sp.label}: L = {v} at {sorted(at)[:6]}"
        rest = np.ones(L.shape, bool)
        for p in want:
            rest[p] = False
        assert np.abs(L[rest]).max() <= 3 * members < 127, f"{name}, {sp.label}: L leaves the benign range elsewhere"
        if members > 1:
            assert np.abs(res).max() <= 65, f"{name}, {sp.label}: a member of an L group near int8's edge"
        hit |= set(want.values())
        # the designed chroma samples: under both luma units of a chroma unit, in the last luma cell of a row, in words 0 and 15
        cw = plane_dims(geom, 1)[0]
        for cy, cx, _ in sp.lsets:
            assert cx < cw and (cx << geom.xd) < geom.w
    assert hit == set(VALUES)
    if members > 1 and geom.xd and GEOMS[name][1] == "wide":  # (cells of 128 samples are the wide chain's)
        cols = {sp.label.rsplit(" ", 1)[0]: {(cx << geom.xd) // UNIT_W - 2 * (cx // UNIT_W) for _, cx, _ in sp.lsets} for sp in sps if sp.section == "B"}
        assert cols["L under the first luma unit"] == {0} and cols["L under the second luma unit"] == {1}, cols
        last = {cx for sp in sps if sp.label.startswith("L last cell") for _, cx, _ in sp.lsets}
        gxc = -(-plane_dims(geom, 1)[0] // UNIT_W)
        assert all(cx // UNIT_W == gxc - 1 and (cx << geom.xd) // UNIT_W == -(-geom.w // UNIT_W) - 1 for cx in last)
        assert gxc * UNIT_W > plane_dims(geom, 1)[0], f"{name}: the last chroma cell of a row is whole"


def _roles(flat, ub: int, counts, poked):
    """What the poked units are to the slices the counts cut."""
    units = unit_list(flat, ub)
    index = {(by, c): i for i, (by, c, _, _) in enumerate(units)}
    roles = set()
    for wgs in counts:
        pos = 0
        for sl in slices(units, wgs):
            first, end = pos, pos + len(sl)
            pos = end
            if not sl:
                continue
            for u in poked:
                i = index[u]
                if i == first - 1 and sl[0][2]:
                    roles.add("ghost in front")
                if i == end and sl[-1][3]:
                    roles.add("ghost behind")
                if i == end - 1 and len(sl) % 2 == 1:
                    roles.add("last of an odd slice")
                if first < i < end - 1:
                    roles.add("interior")
                if i == first:
                    roles.add("first")
    return roles


@pytest.mark.parametrize("name", [n for n, (_, chain) in GEOMS.items() if chain == "wide"])
def test_the_poked_units_sit_at_the_ends_of_slices_and_inside_them(name):
    geom = GEOMS[name][0]
    flat = _flat(_job(name)[2][0])
    want = {"ghost in front", "ghost behind", "last of an odd slice", "interior", "first"}
    for kind in ((0, 1) if geom.chroma else (0,)):
        ub = UNIT_W // plane_dims(geom, kind)[2]
        ncell = len(unit_list(np.ones_like(flat), ub))
        counts = [w_wgs_per_frame(ncell, kind, int(w[kind])) for w in WGS["wide"]]
        have = _roles(flat, ub, counts, _whole_units(geom, kind))
        assert want <= have, f"{name}, kind {kind}: the poked units are never {sorted(want - have)}"


# ---- D ---------------------------------------------------------------------------------------------------------------------------

def _mean_d2(fields, c):
    return float(np.mean([np.mean(np.asarray(f[c], np.float64) ** 2) for f in fields]))


@pytest.mark.parametrize("name", list(BOUNDS))
def test_the_bound_cases_cut_slices_of_the_caps_length(name):
    b = BOUNDS[name]
    fields, _, shadows = _bound_job(name)
    env = dict(b.env)
    for sh in shadows:
        flat = _flat(sh)
        assert flat.all(), f"{name}: {int((~flat).sum())} blocks not flat"
        S_luma = sh["ar"][0][0]
        assert np.abs(S_luma).max() > 2 ** 32, f"{name}: the largest luma S entry is {np.abs(S_luma).max():.3g}"
        if b.chain == "wide":
            ub = UNIT_W // plane_dims(b.geom, b.kind)[2]
            units = unit_list(flat, ub)
            assert len(units) == b.units
            cap = K_W_MAX_UNITS_C if b.kind else K_W_MAX_UNITS
            wgs = w_wgs_per_frame(len(units), b.kind, int(env["G1S_W_WGS_C" if b.kind else "G1S_W_WGS"]))
            sl = slices(units, wgs)
            longest = max(len(s) for s in sl)
            assert longest == b.longest <= cap
            if name == "wide_luma_over":
                assert wgs == 4 and b.units > 3 * cap, "one row of cells over three workgroups' cap: a fourth workgroup"
            else:
                assert wgs == 3 and [len(s) for s in sl] == [cap] * 3
                assert w_wgs_per_frame(len(units), b.kind, 1) == 3  # (what G1S_W_WGS = 1 is raised to)
                mid = sl[1]
                assert mid[0][2] and mid[-1][3], f"{name}: the middle slice has no ghost in front / behind"
                assert sl[0][-1][3] and sl[2][0][2]
            # a wave's accumulator over the slice: units x steps x 64 samples x mean d^2 (the header's 100 x 16 x 64 x 128^2)
            _, _, _, bh = plane_dims(b.geom, b.kind)
            steps = (2 if b.kind else 1) * bh * 2 // 4
        else:
            n_general, n_plain = stream_lists(flat, b.geom)
            assert n_general + n_plain == b.units
            wgs = m_wgs_per_frame(b.units, b.frames, int(env["G1S_F_WGS"]))
            assert wgs == 8
            per_wg = stream_slices(n_general, n_plain, wgs)
            longest = max(per_wg)
            assert sum(per_wg) == b.units and 0.9 * (K_M_MAX_UNITS - 16) <= longest <= K_M_MAX_UNITS, per_wg
            assert longest >= b.longest
            steps = 8  # the luma launch: 32 rows over four waves, 64 samples a step
        bound = longest * steps * 64 * _mean_d2(fields, b.kind if b.chain == "wide" else 0)
        print(f"{name}: longest slice {longest}, {steps} steps a unit, mean d^2 {_mean_d2(fields, b.kind if b.chain == 'wide' else 0):.1f}: {bound:.4g} = 2^{np.log2(bound):.3f}")
        assert bound < 2 ** 31
        if b.chain == "wide" and b.kind:
            # the chroma cap allows no more than 32 units x steps x 64 x 128^2: 2^29 with 16 steps a unit, 2^30 with 32 (the header's
            # case); a field of -128 / 127 has a mean d^2 of 0.992 x 2^14, so the slice comes within a hundredth of that
            assert bound > 0.99 * K_W_MAX_UNITS_C * steps * 64 * 2 ** 14 >= 0.99 * 2 ** 29, f"{name}: {bound:.4g}"
        else:
            assert bound > 2 ** 30, f"{name}: {bound:.4g}"  # the top two bits of an accumulator are live


# ---- each kind of case bites -----------------------------------------------------------------------------------------------------

def _record_of(shadow, geom):
    """A record that holds a shadow's integers (as tests.helpers.record_from_oracle fills one from a live oracle)."""
    from grav1synth_amd.diff import Record

    nplanes = len(shadow["ar"])
    r = Record.blank(geom.w, geom.h, geom.xd, geom.yd, nplanes, geom.lag)
    for c in range(nplanes):
        v = r.views(c)
        S, Sb, nobs = shadow["ar"][c]
        v["S"][:] = S
        v["Sb_nobs"][:-1] = Sb
        v["Sb_nobs"][-1] = nobs
        ls, sd, sd2 = shadow["stats"][c]
        if c == 0:
            v["luma_sum"][:] = ls
            v["mask"][:] = shadow["mask"].ravel()
            v["scores"][:] = shadow["scores"].ravel()
        v["sum_d"][:] = sd
        v["sum_d2"][:] = sd2
    return r


def _wrap8(d):
    return ((np.asarray(d, np.int64) + 128) & 0xff) - 128


def _frame_of(name, label):
    sps, _, shadows = _job(name)
    k = [sp.label for sp in sps].index(label)
    return k, sps[k], shadows[k]


def test_a_wrapped_residual_is_seen():
    """A: the oracle fed the frame with the poked 128 kept as int8 (-128): sum_d2 stays, sum_d and every cross product move.  (The
    builder reaches -128 from a source of 127 and 128 from one of 128, so the reference's luma_sum moves as well, and with the luma
    residual the L of both chroma systems.)"""
    name = "8b420"
    geom = GEOMS[name][0]
    k, sp, right = _frame_of(name, "Y interior 128")
    assert not record_mismatches(right, _record_of(right, geom), "same")
    wrong = _run_oracle(geom, [[_wrap8(p) for p in residuals(geom, k, sp)]])[1][0]
    got = record_mismatches(right, _record_of(wrong, geom), "wrapped")
    print("\n".join(got))
    assert any("plane 0: AR sums differ: S, Sb" in m for m in got) and any("plane 0: block noise sums differ: sum_d (" in m for m in got), got
    assert not any("sum_d2" in m or "mask" in m or "score" in m for m in got), got


def test_a_wrapped_luma_sum_is_seen():
    """B: the chroma planes' sums from the oracle fed a luma whose sums under the designed chroma samples are the wrapped L (128 ->
    -128); the luma plane's own sums left as they are: the L row and column of both chroma systems move."""
    name = "8b420"
    geom = GEOMS[name][0]
    k, sp, right = _frame_of(name, "L under the first luma unit 128")
    res = residuals(geom, k, sp)
    for cy, cx, v in sp.lsets:
        IC.set_L(res[0], cy, cx, int(_wrap8(v)), geom.xd, geom.yd)
    other = _run_oracle(geom, [res])[1][0]
    wrong = dict(right, ar=[right["ar"][0], other["ar"][1], other["ar"][2]])
    got = record_mismatches(right, _record_of(wrong, geom), "wrapped L")
    print("\n".join(got))
    assert len(got) == 2 and all(f"plane {c}: AR sums differ: S, Sb" in m for c, m in zip((1, 2), got)), got


def test_a_sum_reduced_mod_2_32_is_seen():
    """D: S mod 2^32."""
    b = BOUNDS["wide_luma_100"]
    right = _bound_job("wide_luma_100")[2][0]
    S, Sb, nobs = right["ar"][0]
    wrong = dict(right, ar=[(S & 0xffffffff, Sb, nobs)])
    got = record_mismatches(right, _record_of(wrong, b.geom), "mod 2^32")
    print("\n".join(got))
    assert got == ["mod 2^32 plane 0: AR sums differ: S (nobs %d vs %d)" % (nobs, nobs)], got
