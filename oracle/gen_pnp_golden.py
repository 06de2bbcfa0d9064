#!/usr/bin/env python
"""Writes tests/golden/pnp_noise.npz: every problem of tests/pnp_cases.py solved by oracle/pnp_ref.py.

Per population `<name>.<field>`: X, uv, R_true, t_true (the inputs), R, t (the oracle's pose), include (the mask
tests/pnp_cases.py describes), cost (the oracle's squared reprojection error), cost_true (the minimum scipy's MINPACK LM
reaches from the TRUE pose, tests/test_host.py::_scipy_pnp), ratio and cond (lambda1 / lambda2 of the DLT normal matrix,
cond of the DLT rotation block), behind (0 / 1 / 2: pnp_cases.behind of the oracle's pose).  Deterministic: running it
again reproduces the committed file (`--check` compares instead of writing).  Needs numpy and scipy, no GPU."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def generate():
    import pnp_cases as P
    from test_host import _scipy_pnp
    out = {}
    for name in P.POPULATIONS:
        pop = P.population(name)
        n = len(pop['uv'])
        R, t, inc, cost = np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros(n, bool), np.zeros(n)
        cost_true, ratio, cond, beh = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, np.int8)
        for i in range(n):
            R[i], t[i], inc[i], cost[i] = P.solve(name, i)
            cost_true[i] = _scipy_pnp(pop['X'], pop['uv'][i], P.K, pop['R_true'][i], pop['t_true'][i])[2]
            ratio[i], cond[i] = P.dlt_diagnostics(pop['X'], pop['uv'][i])
            beh[i] = P.behind(pop['X'], R[i], t[i]) if inc[i] else 0
        excluded = 1.0 - inc.mean()
        print('%-8s N=%2d sigma=%4.1f px  n=%3d  excluded %2d (%.2f %%)  behind %2d straddling %2d  max l1/l2 %.3f  '
              'max cond(RR) %.2e' % (name, P.POPULATIONS[name][0], P.POPULATIONS[name][1], n, n - inc.sum(), 100 * excluded,
                                     (beh == 1).sum(), (beh == 2).sum(), ratio.max(), cond.max()))
        assert excluded <= P.EXCLUDE_CAP, "%s: %.1f %% excluded - change the seed, not the cap" % (name, 100 * excluded)
        for field, a in dict(pop, R=R, t=t, include=inc, cost=cost, cost_true=cost_true, ratio=ratio, cond=cond,
                             behind=beh).items():
            out['%s.%s' % (name, field)] = a
    return out


def main():
    import pnp_cases as P
    out = generate()
    if sys.argv[1:] == ['--check']:
        z = np.load(P.FIXTURE)
        assert sorted(z.files) == sorted(out)
        for k in out:
            assert np.array_equal(z[k], out[k], equal_nan=out[k].dtype != bool), k
        print('%s reproduced' % os.path.relpath(P.FIXTURE, ROOT))
        return
    np.savez_compressed(P.FIXTURE, **out)
    print('wrote %s (%d bytes)' % (os.path.relpath(P.FIXTURE, ROOT), os.path.getsize(P.FIXTURE)))


if __name__ == '__main__':
    main()
