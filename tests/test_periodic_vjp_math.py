"""CPU checks of the periodic solve's reverse mode: the dense numpy adjoint (tests/periodic_vjp_ref.py)
against directional derivatives of tests/periodic_ref.solve -- 30-digit mpmath for S <= 3 (recorded in
tests/golden/periodic_vjp_dir30.json, the cheapest loops recomputed here), fp64 differences for S = 5 -- and the
identities the gradients obey whatever the reference."""
import numpy as np
import pytest

from tests import periodic_ref, synth
from tests import periodic_vjp_ref as R

# adjoint vs directional derivatives, max-abs error over max-abs reference: 10 x the worst measured over S in {1,2,3,5},
# w in {0, 0.3}, J_bar in {0, 0.7}.  Measured (waypoints / times): order 2 5.3e-15 / 3.5e-12, order 3 2.5e-14 / 2.0e-11,
# order 4 1.9e-11 / 5.2e-10, order 5 1.4e-8 / 3.6e-8 -- the dense fp64 inverses of M in the adjoint and, at S = 5, the
# fp64 difference quotients
GATE_WP = {2: 6e-14, 3: 3e-13, 4: 2e-10, 5: 1.4e-7}
GATE_T = {2: 4e-11, 3: 2e-10, 4: 6e-9, 5: 4e-7}
# the adjoint's coefficients (synth.rel_err_per_power) and J against periodic_ref.solve in fp64, 10 x the worst measured
# over S in {1,2,3,5}, w in {0, 0.3}.  Measured: coefficients 4.7e-15 / 2.6e-13 / 2.5e-10 / 1.5e-6,
# J 4.0e-15 / 1.1e-13 / 9.2e-13 / 5.2e-10 at orders 2 / 3 / 4 / 5 (two dense fp64 solves of different systems)
GATE_COEFFS = {2: 5e-14, 3: 3e-12, 4: 3e-9, 5: 1.5e-5}
GATE_COST = {2: 4e-14, 3: 1.2e-12, 4: 1e-11, 5: 6e-9}
# the two identities, residual over the largest term, 10 x the worst measured over the same loops.  Measured: translation
# 4.0e-16 / 9.8e-15 / 5.2e-13 / 5.9e-11, time scaling 1.1e-15 / 2.1e-14 / 3.5e-13 / 3.6e-10
GATE_TRANSLATION = {2: 4e-15, 3: 1e-13, 4: 6e-12, 5: 6e-10}
GATE_SCALING = {2: 1.1e-14, 3: 2.1e-13, 4: 3.5e-12, 5: 3.6e-9}
JBARS = (0.0, 0.7)

_CASES = None


def _golden():
    global _CASES
    if _CASES is None:
        _CASES = R.golden_cases()
    return _CASES


def _rel(got, ref):
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_adjoint_matches_recorded_30_digit_derivatives(order):
    cases = [c for c in _golden() if c["order"] == order]
    assert sorted({(c["S"], c["w"]) for c in cases}) == [(S, w) for S in (1, 2, 3) for w in (0.0, 0.3)]
    worst = np.zeros(2)
    for c in cases:
        for jb in JBARS:
            r = R.adjoint(order, c["path"], c["time"], c["pbar"], jb, c["w"])
            e_wp = _rel(r["waypoints"], c["wp_p"] + jb * c["wp_J"])
            if c["S"] == 1:   # no time enters a one-point loop: both sides are zero
                assert np.all(r["times"] == 0.0) and np.max(np.abs(c["t_p"] + jb * c["t_J"])) < 1e-25
                e_t = 0.0
            else:
                e_t = _rel(r["times"], c["t_p"] + jb * c["t_J"])
            worst = np.maximum(worst, [e_wp, e_t])
    print("order %d, S <= 3 at 30 digits: waypoints %.2e times %.2e" % (order, worst[0], worst[1]))
    assert worst[0] < GATE_WP[order] and worst[1] < GATE_T[order], worst


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_adjoint_matches_fp64_differences_s5(order):
    path, time, pbar = R.golden_inputs(order, 5)
    worst = np.zeros(2)
    for w in (0.0, 0.3):
        d = R.directional_parts(order, path, time, pbar, w, None)
        for jb in JBARS:
            r = R.adjoint(order, path, time, pbar, jb, w)
            worst = np.maximum(worst, [_rel(r["waypoints"], d["wp_p"] + jb * d["wp_J"]), _rel(r["times"], d["t_p"] + jb * d["t_J"])])
    print("order %d, S = 5 in fp64: waypoints %.2e times %.2e" % (order, worst[0], worst[1]))
    assert worst[0] < GATE_WP[order] and worst[1] < GATE_T[order], worst


@pytest.mark.parametrize("order,S", [(2, 2), (3, 2), (2, 1)])
def test_record_is_what_the_30_digit_solve_gives(order, S):
    """The cheapest recorded loops, recomputed: the record holds periodic_ref's derivatives and the inputs it names."""
    path, time, pbar = R.golden_inputs(order, S)
    for c in (c for c in _golden() if (c["order"], c["S"]) == (order, S)):
        assert np.array_equal(c["path"], path) and np.array_equal(c["time"], time) and np.array_equal(c["pbar"], pbar)
        d = R.directional_parts(order, path, time, pbar, c["w"], 30)
        for k in ("wp_p", "wp_J", "t_p", "t_J"):
            assert np.allclose(d[k], c[k], rtol=1e-12, atol=1e-25), (k, c["w"])


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_adjoint_forward_is_the_periodic_solve(order):
    worst = np.zeros(2)
    for S in (1, 2, 3, 5):
        path, time, pbar = R.golden_inputs(order, S)
        for w in (0.0, 0.3):
            r = R.adjoint(order, path, time, pbar, 0.0, w)
            c, J, _ = periodic_ref.solve(order, path, time, w)
            e_c = synth.rel_err_per_power(r["coeffs"][None], c[None])
            e_J = abs(r["cost"] - J) / J if S > 1 else abs(r["cost"] - J)
            worst = np.maximum(worst, [e_c, e_J])
    print("order %d: coefficients %.2e cost %.2e" % (order, worst[0], worst[1]))
    assert worst[0] < GATE_COEFFS[order] and worst[1] < GATE_COST[order], worst


@pytest.mark.parametrize("order", [2, 3, 4, 5])
@pytest.mark.parametrize("S", [1, 2, 3, 5])
def test_translation_and_scaling_identities(order, S):
    """A translation of the loop moves every constant coefficient and nothing else: sum_k dL/dP_k = sum_j p_bar_j[power 0].
    Scaling every time by s scales the coefficient of power i by s^-i and J by s^(1-2o) (w = 0):
    sum_j T_j T_bar_j = -sum pow_i p_i p_bar_i + (1-2o) J J_bar."""
    m = 2 * order
    path, time, pbar = R.golden_inputs(order, S)
    pw = np.arange(m - 1, -1, -1.0)
    for w in (0.0, 0.3):
        for jb in JBARS:
            r = R.adjoint(order, path, time, pbar, jb, w)
            lhs, rhs = r["waypoints"].sum(axis=0), pbar[:, :, m - 1].sum(axis=0)
            assert np.max(np.abs(lhs - rhs)) < GATE_TRANSLATION[order] * np.max(np.abs(r["waypoints"])), (w, jb)
            if w == 0.0 and S > 1:
                lhs = float(np.sum(time * r["times"]))
                terms = np.array([-np.sum(pw * r["coeffs"] * pbar), (1 - m) * r["cost"] * jb])
                scale = max(np.max(np.abs(time * r["times"])), np.max(np.abs(terms)))
                assert abs(lhs - terms.sum()) < GATE_SCALING[order] * scale, (lhs, terms)


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_single_point_loop_closed_form(order):
    m = 2 * order
    path, time, pbar = R.golden_inputs(order, 1)
    for w, jb in ((0.0, 0.0), (0.3, 0.7)):
        r = R.adjoint(order, path, time, pbar, jb, w)
        assert np.all(r["times"] == 0.0)
        assert np.allclose(r["waypoints"][0], pbar[0, :, m - 1], rtol=1e-12, atol=0.0)
        assert r["cost"] == 0.0 and np.array_equal(r["coeffs"][0, :, m - 1], path[0]) and not r["coeffs"][0, :, :m - 1].any()


def test_adjoint_batch_layouts():
    order, m = 3, 6
    rng = np.random.default_rng(0)
    lens = np.array([3, 0, 1, 2])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    wp, tm = rng.normal(size=(6, 3)), rng.uniform(0.5, 2.0, size=6)
    pbar, jb, w = rng.normal(size=(6, 3, m)), rng.normal(size=4), rng.uniform(0, 0.5, size=4)
    gwp, gt = R.adjoint_batch(order, wp, tm, pbar, jb, w, seg_offsets=off)
    assert gwp.shape == (6, 3) and gt.shape == (6,)
    for b in (0, 2, 3):
        r = R.adjoint(order, wp[off[b]:off[b + 1]], tm[off[b]:off[b + 1]], pbar[off[b]:off[b + 1]], jb[b], w[b])
        assert np.array_equal(gwp[off[b]:off[b + 1]], r["waypoints"]) and np.array_equal(gt[off[b]:off[b + 1]], r["times"])
    u_wp, u_t = R.adjoint_batch(order, wp.reshape(2, 3, 3), tm.reshape(2, 3), pbar.reshape(2, 3, 3, m), None, 0.2)
    assert u_wp.shape == (2, 3, 3) and u_t.shape == (2, 3)
    assert np.array_equal(u_wp[1], R.adjoint(order, wp[3:], tm[3:], pbar[3:], 0.0, 0.2)["waypoints"])
