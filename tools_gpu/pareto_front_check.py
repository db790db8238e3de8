#!/usr/bin/env python3
"""ParetoFront.update(DevicePopulation) at archive sizes the test suite cannot
afford (its oracle there is a Python loop): two objectives on a synthetic
front, four successive updates of up to 2^17 rows with many equal genomes,
checked row for row against a numpy statement of the closed form (DESIGN §11:
a sweep over the lexicographic order for the members, a dict for the twins, a
stable sort for the order).  Prints each update's sizes and wall time."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from deap_amd import tools  # noqa: E402
from deap_amd.device import DevicePopulation  # noqa: E402


def oracle(Hg, Hw, Pg, Pw):
    g = np.concatenate([Hg, Pg]); w = np.concatenate([Hw, Pw]) + 0.0
    nH = len(Hg)
    order = np.lexsort((-w[:, 1], -w[:, 0]))
    alive = np.zeros(len(w), bool)
    best1 = -np.inf; i = 0
    while i < len(order):
        j = i
        while j < len(order) and w[order[j], 0] == w[order[i], 0]:
            j += 1
        top = w[order[i], 1]
        if top > best1:
            for k in range(i, j):
                if w[order[k], 1] == top:
                    alive[order[k]] = True
            best1 = top
        i = j
    seen = set(); keep = []
    for s in np.nonzero(alive)[0]:
        key = (w[s].tobytes(), (g[s] + 0.0).tobytes())
        if s >= nH and key in seen:
            continue
        seen.add(key); keep.append(s)
    keep = np.array(keep)
    # layout: new rows by descending row, then H in order; stable sort desc
    new = keep[keep >= nH][::-1]; old = keep[keep < nH]
    lay = np.concatenate([new, old])
    o = np.lexsort((-w[lay, 1], -w[lay, 0]))  # lexsort is stable
    lay = lay[o]
    return g[lay], w[lay]


rng = np.random.default_rng(0)
pf = tools.ParetoFront()
Hg = np.zeros((0, 3)); Hw = np.zeros((0, 2))
for u, n in enumerate((100000, 131072, 70001, 5)):
    x = np.round(rng.uniform(0, 1, n), 4)
    slack = np.where(rng.random(n) < 0.1, 0.0, np.round(rng.uniform(0, 0.3, n) / (u + 1), 4))
    w = np.stack([x, np.round(1 - x * x, 4) - slack], 1)
    g = rng.integers(0, 3, (n, 3)).astype(np.float64)
    pop = DevicePopulation.from_numpy(g, weights=(1.0, 1.0), gtype="f64", wvalues=w, valid=np.ones(n))
    t = time.time(); pf.update(pop); pop.ctx.sync(); dt = time.time() - t
    Hg, Hw = oracle(Hg, Hw, g, w)
    dg, dw, ok = pf.front().to_numpy()
    same = len(dg) == len(Hg) and np.array_equal(dg, Hg) and np.array_equal(dw, Hw)
    print("update %d: n=%d front device %d oracle %d same=%s %.1f ms" % (u, n, len(pf), len(Hg), same, dt * 1e3), flush=True)
    assert same
print("ok")
