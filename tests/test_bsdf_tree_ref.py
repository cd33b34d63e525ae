"""The float64 restatement of tests/bsdf_tree_ref.py, checked on the CPU before any device value is looked at:

  a. against the oracle where the oracle can speak -- plain, untextured, unwrapped leaves on the rectangle, the disk and the quad, hit
     from both sides under the chromatic `constant` emitter, 4 096 lanes per case, for `path`, `volpath` rgb and `volpath` mono:
     this fixes the draw offsets and validates the MIS, leaf and warp restatements; and the leaves alone against the oracle's BSDFs;
  b. the fp32 scale E of that comparison, measured here, against the constants the device bound is made of;
  c. the lanes the reference leaves out: at most 2 % of every case, every branch still populated, both terms alive;
  d. teeth: every mutation of the restatement differs from the true one by more than the device test allows on >= 5 % of some case's lanes.

Every figure printed here is measured on the CPU."""
import numpy as np
import pytest

import tests.bsdf_tree_ref as R
import tests.oracle_binding as ob

N_ORACLE = 4096
INTEGRATORS = [("path", False), ("volpath", False), ("volpath", True)]
# Bound of section a: the oracle evaluates the same expression in fp32 -- some fifty operations and two powers per lane, each good
# to an ulp or a few (2^-24 = 6e-8) -- so 1e-5 of the value's scale is two orders above what can accumulate and three below the
# several percent of a wrong offset, MIS weight, lobe or warp.  Section b holds the measured figure itself.
ORACLE_TOL = 1e-5

_CASES, _ORACLE = {}, {}


def case_of(name, surface, placement, n=R.N_LANES, trees=None, expanded=False):
    key = (name, surface, placement, n, expanded, id(trees or R.ALL_TREES))
    if key not in _CASES:
        _CASES[key] = R.build_case((trees or R.ALL_TREES)[name], surface, placement, expanded=expanded, n=n)
    return _CASES[key]


def oracle_errors(leaf, surface, placement, integrator, mono):
    """computed once per case, shared by sections a and b, left unchanged -> (scaled error (n, 3), restatement, oracle rgb, valid)"""
    key = (leaf, surface, placement, integrator, mono)
    if key not in _ORACLE:
        case = case_of(leaf, surface, placement, N_ORACLE, R.GREY_LEAVES if mono else R.LEAVES, expanded=True)
        scene = dict(case.scene, integrator=dict(case.scene["integrator"], type=integrator))
        rgb, valid = ob.OracleScene(scene, mono=mono).sample(case.origins, case.directions, seed_offset=R.SEED_OFFSET)
        ref = R.restate(case, integrator=integrator, mono=mono)
        _ORACLE[key] = (R.scaled_error(rgb, ref.value), ref, rgb, valid)
    return _ORACLE[key]


# ================================================================ a. the restatement against the oracle
@pytest.mark.parametrize("integrator,mono", INTEGRATORS)
@pytest.mark.parametrize("surface,placement", R.SHEETS)
@pytest.mark.parametrize("leaf", sorted(R.LEAVES))
def test_restatement_agrees_with_the_oracle(leaf, surface, placement, integrator, mono):
    err, ref, rgb, valid = oracle_errors(leaf, surface, placement, integrator, mono)
    kept = ref.kept
    print("%s %s %s %s%s: kept %d of %d, max scaled error %.3g" % (leaf, surface, placement, integrator, " mono" if mono else "", kept.sum(), len(kept), err[kept].max()))
    assert valid.all()
    assert np.array_equal(rgb[kept] == 0, ref.value[kept] == 0)             # the lanes and channels without light are the same
    assert err[kept].max() <= ORACLE_TOL
    assert (ref.value[kept] > 0).any(axis=1).mean() > 0.3


@pytest.mark.parametrize("integrator,mono,wrong", [("path", False, 1), ("volpath", False, 1), ("volpath", False, 3), ("volpath", True, 0), ("volpath", True, 2)])
def test_a_wrong_draw_offset_is_rejected(integrator, mono, wrong, monkeypatch):
    """what decides the offsets: with the stream shifted by one draw either way the restatement is another sample altogether"""
    err, ref, rgb, valid = oracle_errors("rpv", "rectangle", None, integrator, mono)
    assert wrong != R.STREAM_OFFSET[(integrator, mono)]
    monkeypatch.setitem(R.STREAM_OFFSET, (integrator, mono), wrong)
    shifted = R.restate(case_of("rpv", "rectangle", None, N_ORACLE, R.GREY_LEAVES if mono else R.LEAVES, expanded=True), integrator=integrator, mono=mono)
    share = (R.scaled_error(rgb, shifted.value).max(axis=1) > ORACLE_TOL)[ref.kept & shifted.kept].mean()
    print("%s%s at offset %d: %.1f %% of the lanes differ" % (integrator, " mono" if mono else "", wrong, 100 * share))
    assert share > 0.5


@pytest.mark.parametrize("leaf", sorted(R.LEAVES))
def test_leaves_agree_with_the_oracle(leaf):
    """eval, pdf and sample of a leaf alone against oracle_bsdf_eval / oracle_bsdf_sample, wi and wo on both sides"""
    n = 256
    rng = np.random.default_rng(5)
    case = case_of(leaf, "rectangle", None, N_ORACLE, R.LEAVES, expanded=True)
    o = ob.OracleScene(case.scene)
    assert o.desc.bsdf_count == 1
    v = rng.normal(size=(2, n, 3))
    v /= np.linalg.norm(v, axis=2)[..., None]
    ok = (np.abs(v[0][:, 2]) >= R.WI_MARGIN) & (np.abs(v[1][:, 2]) >= R.HORIZON_MARGIN)
    wi, wo = R.f32(v[0][ok]), R.f32(v[1][ok])
    s = R.f32(rng.random((len(wi), 3)))
    ev = R.Evaluator(R.LEAVES[leaf], np.zeros((len(wi), 2)))
    val, pdf = ev.eval_pdf(wi, wo)
    bs = ev.sample(wi, s[:, 0], s[:, 1:])
    scale = lambda a: np.abs(a) + 1.0
    worst = 0.0
    for i in range(len(wi)):
        ov, op = o.bsdf_eval(0, wi[i], wo[i])
        worst = max(worst, (np.abs(ov - val[i]) / scale(val[i])).max(), abs(op - pdf[i]) / scale(pdf[i]))
        assert np.array_equal(ov == 0, val[i] == 0) and (op == 0) == (pdf[i] == 0)
        if bs.threshold[i] < R.THRESHOLD_MARGIN or (abs(bs.wo[i, 2]) < R.HORIZON_MARGIN and bs.pdf[i] != 0):
            continue
        owo, opdf, ow, _ = o.bsdf_sample(0, wi[i], float(s[i, 0]), (float(s[i, 1]), float(s[i, 2])))
        worst = max(worst, np.abs(owo - bs.wo[i]).max(), abs(opdf - bs.pdf[i]) / scale(bs.pdf[i]), (np.abs(ow - bs.weight[i]) / scale(bs.weight[i])).max())
        assert np.array_equal(ow == 0, bs.weight[i] == 0)
    print("%s alone: max error %.3g over %d directions" % (leaf, worst, len(wi)))
    assert worst <= ORACLE_TOL
    if leaf != "diffuse":
        assert (val > 0).any()
    assert (bs.weight > 0).any() and (bs.weight == 0).all(axis=1).any() == (leaf != "bilambertian")


# ================================================================ b. the fp32 scale E
def measured_scale(world):
    worst = 0.0
    for leaf in sorted(R.LEAVES):
        for surface, placement in R.SHEETS:
            if (placement is not None) != world:
                continue
            for integrator, mono in INTEGRATORS:
                err, ref, _, _ = oracle_errors(leaf, surface, placement, integrator, mono)
                worst = max(worst, err[ref.kept].max())
    return worst


def test_the_fp32_scale_is_within_its_constants():
    """E, measured afresh on the CPU from the oracle, against the committed constants (the device bound is DEVICE_FACTOR times them)"""
    canonical, world = measured_scale(False), measured_scale(True)
    print("E measured on the CPU: canonical sheets %.4g (constant %.4g), world-space sheets %.4g (constant %.4g); device bounds %.4g / %.4g"
          % (canonical, R.E_CANONICAL, world, R.E_WORLD, R.DEVICE_FACTOR * R.E_CANONICAL, R.DEVICE_FACTOR * R.E_WORLD))
    assert canonical <= R.E_CANONICAL and world <= R.E_WORLD
    assert R.E_CANONICAL <= 2.0 * canonical and R.E_WORLD <= 2.0 * world     # and the constants are that measurement, not a loose guess


# ================================================================ c. lanes the reference leaves out
ALL_CASES = [(name, surface, placement) for name in R.ALL_TREES for surface, placement in R.SHEETS]


@pytest.mark.parametrize("name,surface,placement", ALL_CASES)
def test_few_lanes_are_left_out_and_every_branch_is_met(name, surface, placement):
    case = case_of(name, surface, placement)
    for integrator, mono in INTEGRATORS:
        ref = R.restate(case, integrator=integrator, mono=mono)
        kept = ref.kept
        dropped = 1.0 - kept.mean()
        both = ((ref.emitter_term[kept] != 0).any(axis=1) & (ref.bsdf_term[kept] != 0).any(axis=1)).mean()
        print("%s %s %s %s%s: dropped %.3f %%, both terms alive on %.1f %% of the kept lanes" % (name, surface, placement, integrator, " mono" if mono else "", 100 * dropped, 100 * both))
        assert dropped <= R.MAX_DROP
        assert both >= 0.25
        assert np.isfinite(ref.value[kept]).all()
        for tag, values in R.expected_branches(case.tree).items():
            assert set(np.unique(ref.tags[tag][kept])) - {-1} == values, tag


@pytest.mark.parametrize("name,surface,placement", R.BACKDROP_CASES)
def test_the_backdrop_case_keeps_its_lanes(name, surface, placement):
    """every lane meets the back; the backdrop changes no value (no path that carries light reaches it) and costs few lanes"""
    case = case_of(name, surface, placement)
    ref = R.restate(case)
    kept = ref.kept
    both = ((ref.emitter_term[kept] != 0).any(axis=1) & (ref.bsdf_term[kept] != 0).any(axis=1)).mean()
    print("%s with the backdrop: dropped %.3f %%, both terms alive on %.1f %% of the kept lanes" % (name, 100 * (1.0 - kept.mean()), 100 * both))
    assert 1.0 - kept.mean() <= R.MAX_DROP and both >= 0.25
    assert set(np.unique(ref.tags["twosided_side"][kept])) == {1}
    free = R.sheet_sample(R.Evaluator(case.tree, case.uv), case.normal, case.dp_du, case.directions.astype(np.float64), R.case_uniforms(case.n))
    assert np.array_equal(free.value[kept], ref.value[kept])


def test_the_clamped_weight_reaches_both_ends():
    node = R.Evaluator(R.CATALOGUE["blend_d_d_wclamped"], case_of("blend_d_d_wclamped", "rectangle", None).uv).root
    assert (node["weight"] == 0).any() and (node["weight"] == 1).any() and ((node["weight"] > 0) & (node["weight"] < 1)).any()


# ================================================================ d. teeth
def mutation_shares(mutation):
    """per case (every tree on the plain rectangle and inside the mirrored instance, and the backdrop cases, `path`): the share of
    the kept lanes on which the mutated restatement is further from the true one than the device test allows for that tree"""
    shares = {}
    for name, surface, placement in MUTATION_CASES:
        case = case_of(name, surface, placement)
        true, wrong = R.restate(case), R.restate(case, mutation=mutation)
        shares[(name, surface, placement)] = float(R.exceeds_bound(name, placement, wrong.value, true.value)[true.kept].mean())
    return shares


MUTATION_CASES = [(name, s, p) for name in R.ALL_TREES for s, p in (("rectangle", None), ("quad_uv", "mirrored"))] + R.BACKDROP_CASES


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_is_rejected(mutation):
    shares = mutation_shares(mutation)
    best = max(shares, key=shares.get)
    print("%s: %.1f %% of the kept lanes of %s; by tree: %s" % (mutation, 100 * shares[best], best, ", ".join(
        "%s %.1f" % (name, 100 * max(v for k, v in shares.items() if k[0] == name and k[2] != "backdrop")) for name in R.ALL_TREES)))
    assert shares[best] >= 0.05
