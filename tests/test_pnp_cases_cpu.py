"""The noisy-corner PnP fixture (tests/golden/pnp_noise.npz, tests/pnp_cases.py) pinned on the CPU.  No GPU.

What tests/test_gpu_pnp.py relies on and this file establishes:
  - the fixture is what oracle/pnp_ref.py returns for the seeded populations (a subset is solved again: inputs bit for
    bit, reprojections to 1e-9 px, the same include mask);
  - at most 5 % of any population is excluded (pnp_cases.EXCLUDE_CAP);
  - the oracle's poses are least-squares minima: with every point in front of the camera its cost is never below the
    minimum scipy's MINPACK LM reaches from the TRUE pose by more than 1e-7 relative.  (A mirrored pose, every point
    behind the camera, is another minimum of the same unconstrained objective and can be lower: 0.33 x at the least
    here.  It is still the algorithm's answer, see pnp_cases.)"""
import numpy as np
import pytest

import pnp_cases as P


def _subset(name):
    n = P.POPULATIONS[name][2]
    return range(0, n, 8) if n == 160 else range(0, n, 2)          # 20 / 16 problems


@pytest.mark.parametrize("name", list(P.POPULATIONS))
def test_fixture_is_the_oracles_answer(name):
    d, pop = P.golden()[name], P.population(name)
    N, _, n, _ = P.POPULATIONS[name]
    assert d['uv'].shape == (n, N, 2) and d['R'].shape == (n, 3, 3) and d['t'].shape == (n, 3)
    for k in ('X', 'uv', 'R_true', 't_true'):
        assert np.array_equal(d[k], pop[k]), k
    assert np.array_equal(d['uv'], d['uv'].astype(np.float32).astype(np.float64))      # what the decode hands over
    for i in _subset(name):
        R, t, include, cost = P.solve(name, i)
        assert include == bool(d['include'][i])
        if include:
            assert np.abs(P.reproject(d['X'], R, t) - P.reproject(d['X'], d['R'][i], d['t'][i])).max() < 1e-9
            assert abs(cost - d['cost'][i]) <= 1e-9 * max(cost, 1.0)
            assert P.behind(d['X'], R, t) == d['behind'][i]
        ratio, cond = P.dlt_diagnostics(d['X'], d['uv'][i])
        assert abs(ratio - d['ratio'][i]) < 1e-6 and abs(cond - d['cond'][i]) < 1e-6 * cond


@pytest.mark.parametrize("name", list(P.POPULATIONS))
def test_exclusion_cap(name):
    inc = P.golden()[name]['include']
    assert inc.dtype == bool and len(inc) == P.POPULATIONS[name][2]
    assert 1.0 - inc.mean() <= P.EXCLUDE_CAP, "%s: %d of %d excluded" % (name, (~inc).sum(), len(inc))
    if P.POPULATIONS[name][2] == 160:
        assert len(inc) % 64 != 0


@pytest.mark.parametrize("name", list(P.POPULATIONS))
def test_oracle_cost_against_independent_minimiser(name):
    from test_host import _scipy_pnp
    d = P.golden()[name]
    front = d['include'] & (d['behind'] == 0)
    assert front.sum() >= 0.35 * len(front)
    # the stored minimum is scipy's (subset solved again), and the oracle never undercuts it
    for i in _subset(name):
        c = _scipy_pnp(d['X'], d['uv'][i], P.K, d['R_true'][i], d['t_true'][i])[2]
        assert abs(c - d['cost_true'][i]) <= 1e-9 * max(c, 1.0)
    worst = ((d['cost_true'][front] - d['cost'][front]) / d['cost_true'][front]).max()
    assert worst <= 1e-7, worst
