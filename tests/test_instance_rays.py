"""tests/instance_rays.py without a GPU: the helper is checked against the oracle, the fp32 scale of intersection at these coordinates
is measured, and every condition the device tests (tests/test_gpu_instance_rays.py) rely on is asserted for the committed inputs.

Figures of the committed inputs (printed by the tests; DESIGN.md 2 has them with the device's): E_t = 1.16e-6, E_p = 2.09e-6,
E_n = 1.51e-6 -- the oracle on the expanded dyadic scene against the float64 restatement; 0.05 - 0.8 % of a ray set dropped; the
restatement answers 2.1 % of the rays differently without one mirror and 13 % with one placement's scale and rotation exchanged."""
import numpy as np
import pytest

import tests.instance_rays as ir

SETS = ("aimed", "through", "nadir", "inside")
ATOL = 1e-4                                                            # the textured tests' tolerance (tests/test_gpu_textures.py)


def wins(ref, keep):
    hit = keep & np.isfinite(ref["t"])
    return set(zip(ref["instance"][hit].tolist(), ref["member"][hit].tolist()))


def test_expand_is_defined_for_dyadic_placements_only():
    with pytest.raises(ValueError, match="not placed by a diagonal matrix"):
        ir.expand(ir.general_grove())
    d = ir.dyadic_grove()
    k = next(k for k, p in enumerate(d.spec["places"]) if p[0] == "B")
    d["inst_%03d" % k]["to_world"] = ir.T.translate([0.5, 0.0, 0.0]) @ ir.T.scale([1.0, 2.0, 1.0])
    with pytest.raises(ValueError, match="sphere under an uneven scale"):
        ir.expand(d)


@pytest.mark.parametrize("which", ["dyadic", "dyadic_wide"])
def test_dyadic_placements_are_what_the_exactness_argument_needs(which):
    d = ir.GROVES[which]()
    assert sum(1 for p in d.spec["places"] if p[0] == "A" and np.prod(p[4]) < 0) >= 4
    for g, t, axis, angle, s in d.spec["places"]:
        assert angle == 0.0 and np.all(np.abs(t) <= 2.0) and np.all(np.asarray(t) * 16 == np.round(np.asarray(t) * 16))
        assert set(np.abs(s)) <= {0.5, 1.0, 2.0} and (g == "A" or len(set(np.abs(s))) == 1)
    for members in d.spec["groups"].values():
        for m in members:
            pts = np.asarray(m[1], np.float64)
            assert np.all(pts * 64 == np.round(pts * 64)) and np.abs(pts).max() <= 1.0
            assert np.all(pts[..., :2] * 4 == np.round(pts[..., :2] * 4))            # x, y of vertices and centres: what the nadir origins avoid
            if m[0] in ("rectangle", "disk"):
                assert m[3] == 0.0 and set(m[4]) <= {0.5, 1.0}
    for o, w, mint, maxt in ir.ray_sets(which).values():
        assert np.all(o * 256 == np.round(o * 256)) and np.abs(o).max() <= 4.0
    o, w, _, _ = ir.ray_sets(which)["nadir"]
    assert np.all(w == np.array([0, 0, -1], np.float32))
    assert np.all((o[:, 0] * 256) % 2 == 1) and np.all((o[:, 1] * 32) % 2 == 1)


def test_general_placements():
    d = ir.general_grove()
    places = d.spec["places"]
    assert sum(1 for p in places if np.prod(p[4]) < 0) == len(places) // 3
    assert all(0.5 <= abs(x) <= 2.0 for p in places for x in p[4]) and all(p[3] != 0.0 for p in places)
    boxes = ir.instance_boxes(d)
    assert np.abs(boxes).max() <= 4.0
    for o, w, mint, maxt in ir.ray_sets("general").values():
        assert np.abs(o).max() <= 4.0


def test_oracle_on_the_expanded_scene_against_the_float64_restatement():
    """the member and the instance are identical on every kept ray; E_t, E_p, E_n are what fp32 intersection costs here"""
    e_t, e_p, e_n = ir.fp32_scale()
    print("E_t = %.3g  E_p = %.3g  E_n = %.3g; bounds 8 E: %.3g %.3g %.3g" % (e_t, e_p, e_n, 8 * e_t, 8 * e_p, 8 * e_n))
    assert 0 < 8 * e_t <= ATOL and 0 < 8 * e_p <= ATOL and 0 < 8 * e_n <= ATOL     # a bound above ATOL: the ray selection is wrong
    results, where = ir.expanded_oracle()
    for name in SETS:
        got, ref = results[name], ir.reference("dyadic", name)
        keep = ir.kept(ref, e_t)
        hit = np.isfinite(ref["t"])
        assert np.array_equal(np.isfinite(got["t"])[keep], hit[keep]), name
        k = keep & hit
        assert np.array_equal(where[got["shape"][k], 0], ref["instance"][k]), name
        assert np.array_equal(where[got["shape"][k], 1], ref["member"][k]), name
        assert np.array_equal(got["prim_index"][k], ref["prim"][k]), name
        assert np.all(got["shape"][keep & ~hit] == -1)


@pytest.mark.parametrize("which", ["dyadic", "general"])
def test_conditions_of_the_ray_sets(which):
    e_t = ir.fp32_scale()[0]
    d, prims, boxes, sets = ir._ray_sets(which)
    table = ir.shape_table(d)
    won = set()
    for name in SETS:
        o, w, mint, maxt = sets[name]
        assert len(o) == ir.N_RAYS
        ref = ir.reference(which, name)
        keep = ir.kept(ref, e_t)
        hit = np.isfinite(ref["t"])
        lo, hi = ir.box_spans(boxes, o.astype(np.float64), w.astype(np.float64))
        crossed = ((lo < hi) & (hi >= mint[:, None]) & (lo <= maxt[:, None])).sum(1)
        dropped, hitting, two = 1.0 - keep.mean(), hit[keep].mean(), (crossed[keep & hit] >= 2).mean()
        print("%s %s: dropped %.2f %%, hitting %.1f %% of the kept, %.1f %% of those cross two or more instances' boxes" % (which, name, 100 * dropped, 100 * hitting, 100 * two))
        assert dropped <= 0.03 and hitting >= 0.60 and two >= 0.30
        won |= wins(ref, keep)
    # every member of every instance, and both plain rectangles, win at least once
    want = {(k, m) for k, p in enumerate(d.spec["places"]) for m in table["members"][p[0]]} | {(-1, p) for p in table["plain"]}
    assert want <= won, sorted(want - won)
    if which == "dyadic":
        assert (np.isfinite(sets["inside"][3]).mean() > 0.3) and (sets["inside"][2] > 0.1).mean() > 0.3       # windows at both ends


@pytest.mark.parametrize("which", ["dyadic", "dyadic_wide"])
def test_expanded_oracle_has_no_exact_tie(which):
    """the oracle gives an exact tie in t to the later primitive: with the shapes and every mesh's faces listed the other way round it
    names the same winner on every ray iff no tie occurs -- the device's (scene primitive, group primitive) order need not be either"""
    import tests.oracle_binding as ob
    plain, where = ir.expand(ir.GROVES[which]())
    other, back = ir.reversed_order(plain)
    faces = {i: len(plain[k]["faces"]) for i, k in enumerate(k for k in plain if k[:2] in ("x_", "y_")) if plain[k]["type"] == "mesh"}
    scene = ob.OracleScene(other)
    results = ir.expanded_oracle(which)[0]
    back = np.array(back)
    for name, rays in ir.ray_sets(which).items():
        a, b = results[name], scene.ray_intersect(*rays)
        assert np.array_equal(a["t"].view(np.uint32), b["t"].view(np.uint32)), name
        hit = np.isfinite(a["t"])
        shape = back[b["shape"][hit]]
        assert np.array_equal(shape, a["shape"][hit]), name
        count = np.array([faces.get(s, 0) for s in shape])
        assert np.array_equal(np.where(count > 0, count - 1 - b["prim_index"][hit], b["prim_index"][hit]), a["prim_index"][hit]), name


@pytest.mark.parametrize("kind", ["unmirrored", "order"])
def test_the_restatement_has_teeth(kind):
    """one placement without its mirror, one with scale and rotation exchanged: more than 1 % of the rays get another answer"""
    d = ir.general_grove()
    e_t = ir.fp32_scale()[0]
    refs = {name: ir.reference("general", name) for name in SETS}
    count = np.zeros(len(d.spec["places"]), int)
    for ref in refs.values():
        count += np.bincount(ref["instance"][ref["instance"] >= 0], minlength=len(count))
    mirrored = np.array([np.prod(p[4]) < 0 for p in d.spec["places"]])
    k = int(np.argmax(np.where(mirrored, count, -1) if kind == "unmirrored" else np.where(mirrored, -1, count)))
    prims = ir.world_primitives(d, (kind, k))
    differing = total = 0
    for name in SETS:
        ref = refs[name]
        got = ir.reference_hits(d, *ir.ray_sets("general")[name], prims=prims)
        with np.errstate(invalid="ignore"):
            dt = np.where(np.isfinite(ref["t"]) & np.isfinite(got["t"]), np.abs(got["t"] - ref["t"]), 0.0)
            dn = np.abs(got["n"] - ref["n"]).max(1)
        differing += int(np.sum((got["winner"] != ref["winner"]) | (dt > 8 * e_t) | (dn > 8 * ir.fp32_scale()[2])))
        total += len(dt)
    print("%s of placement %d: %.2f %% of the rays differ" % (kind, k, 100.0 * differing / total))
    assert differing > 0.01 * total


def test_conditions_of_the_shadow_segments():
    """at most 5 % of the segments dropped, at least 30 % of the kept ones occluded; expected radiances within reach of ATOL"""
    d, o, w, expected, keep, visible, beyond = ir.shadow_case()
    assert len(o) == ir.N_SHADOW == 256 and np.abs(o).max() <= 4.0
    print("shadow segments: dropped %.1f %%, occluded %.1f %% of the kept, lit with an occluder beyond the lamp: %d" % (100 * (1 - keep.mean()), 100 * (~visible[keep]).mean(), int((visible & beyond & keep).sum())))
    assert 1.0 - keep.mean() <= 0.05 and (~visible[keep]).mean() >= 0.30 and (visible[keep]).mean() >= 0.30
    assert (visible & beyond & keep).sum() >= 16
    assert expected[visible].min() > 100 * ATOL                           # a missed shadow is far outside the tolerance
    # the sensor rays meet the ground before anything else
    ref = ir.reference_hits(ir.general_grove(), o, w, maxt=np.full(len(o), 0.3))
    assert not np.isfinite(ref["t"]).any()
