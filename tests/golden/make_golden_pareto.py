#!/usr/bin/env python3
"""Generate tests/golden/pareto.npz: the reference's ``tools.ParetoFront``
(deap/tools/support.py:591-640) run over recorded populations — BUILD
container only, like make_golden.py (the reference is loaded through its
``load_reference``; nothing of it is copied, only the data it produces).

Every case is four successive ``update`` calls on one front.  Stored per case
``c`` and update ``u``: ``c/u/pop_genes``, ``c/u/pop_wv`` (the population:
genes as floats or 0/1 bits, weighted values) and ``c/u/front_genes``,
``c/u/front_wv`` (the hall afterwards, in its order), plus ``c/weights`` and
``c/gtype``.

Usage:  python tests/golden/make_golden_pareto.py
"""
import array
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import load_reference  # noqa: E402

SIZES = (1, 7, 300, 513)


def lattice2(rng):
    """2 objectives on a 5x5 integer lattice, 6 genomes: twins inside the
    population, against the archive, and equal fitness with other genomes;
    zeros of either sign."""
    pool = rng.uniform(-1, 1, (6, 5))
    fixed = {}
    gens = []
    for u, n in enumerate(SIZES):
        genes, vals = [], []
        for _ in range(n):
            g = int(rng.integers(6))
            if rng.random() < 0.5 and g in fixed:
                v = fixed[g]
            else:
                a = int(rng.integers(5))
                d = int(rng.integers(max(0, 2 - u), 3))
                v = (float(a), float(max(0, 4 - a - d)))
                fixed.setdefault(g, v)
            v = tuple(-0.0 if x == 0 and rng.random() < 0.5 else x for x in v)
            genes.append(pool[g])
            vals.append(v)
        gens.append((np.array(genes), vals))
    return (1.0, 1.0), "f64", gens


def lattice3(rng):
    """3 objectives, mixed signs, on a 3x3x3 lattice; 70-bit genomes (the row
    crosses a 64-bit word); a zero value under a negative weight is -0.0."""
    pool = rng.integers(0, 2, (6, 70))
    pool[1] = pool[0]
    pool[1, 69] ^= 1  # differs from genome 0 in the second word only
    gens = []
    for u, n in enumerate(SIZES):
        floor = 3 if u < 2 else 2
        genes, vals = [], []
        while len(vals) < n:
            v = rng.integers(0, 3, 3)
            if v[0] + (2 - v[1]) + v[2] < floor:
                continue
            genes.append(pool[int(rng.integers(6))])
            vals.append(tuple(float(x) for x in v))
        gens.append((np.array(genes), vals))
    return (-1.0, 1.0, -1.0), "bits", gens


def wide2(rng):
    """300 mutually non-dominated rows first (the archive crosses a 256-row
    tile); later populations dominate slices of them, re-submit exact copies
    of archive members and add new non-dominated rows."""
    g0 = rng.uniform(0, 1, (300, 3))
    order = rng.permutation(300)
    gens = [(g0[order], [(float(i), float(-i)) for i in order])]
    genes, vals = [], []
    for i in range(100, 150):       # dominate the points 100..149
        genes.append(rng.uniform(0, 1, 3))
        vals.append((i - 0.5, -i - 0.5))
    for i in rng.integers(0, 300, 200):  # exact copies of archive members
        genes.append(g0[i])
        vals.append((float(i), float(-i)))
    while len(vals) < 513:          # between the points: non-dominated (or under a dominator)
        i = int(rng.integers(0, 300))
        genes.append(rng.uniform(0, 1, 3))
        vals.append((i + 0.25, -i - 0.25))
    p = rng.permutation(513)
    gens.append((np.array(genes)[p], [vals[j] for j in p]))
    genes = [g0[7], g0[7], g0[120], rng.uniform(0, 1, 3), rng.uniform(0, 1, 3), g0[299],
             rng.uniform(0, 1, 3)]
    vals = [(7.0, -7.0), (7.0, -7.0), (120.0, -120.0), (199.5, -200.5), (7.0, -7.0),
            (299.0, -299.0), (250.75, -250.75)]
    gens.append((np.array(genes), vals))
    gens.append((rng.uniform(0, 1, (1, 3)), [(-1.0, -1.0)]))  # dominates the points 0 and 1
    return (-1.0, -1.0), "f64", gens


def single(rng):
    """One objective: many rows tie at the maximum with few distinct genomes;
    the whole front is one equal-fitness run."""
    pool = rng.integers(0, 2, (5, 70))
    gens = []
    for u, n in enumerate(SIZES):
        top = 11.0 if u == 3 else 10.0
        genes, vals = [], []
        for k in range(n):
            fresh = rng.random() < 0.2
            genes.append(rng.integers(0, 2, 70) if fresh else pool[int(rng.integers(5))])
            at_top = k == 0 or rng.random() < (0.3 if u == 3 else 0.6)
            vals.append((top if at_top else float(rng.integers(0, 10)),))
        gens.append((np.array(genes), vals))
    return (1.0,), "bits", gens


def nan_gene(rng):
    """Rows with identical bits that hold a NaN gene and share a fitness:
    NaN != NaN, so none is the other's twin and all of them stay."""
    pool = rng.uniform(-1, 1, (4, 4))
    nan_row = np.array([0.5, np.nan, -0.0, 2.0])
    gens = []
    for u, n in enumerate(SIZES):
        genes, vals = [], []
        for k in range(n):
            if n > 1 and k in (2, 5):
                genes.append(nan_row.copy())
                vals.append((0.0, 9.0))
                continue
            a = int(rng.integers(5))
            genes.append(pool[int(rng.integers(4))])
            vals.append((float(a), float(4 - a - int(rng.integers(0, 2)))))
        gens.append((np.array(genes), vals))
    return (1.0, 1.0), "f64", gens


CASES = {"lattice2": lattice2, "lattice3": lattice3, "wide2": wide2, "single": single,
         "nan_gene": nan_gene}


def main():
    mods = load_reference()
    base, creator, tools = mods["deap.base"], mods["deap.creator"], mods["deap.tools"]
    out = {}
    for ci, (name, make) in enumerate(CASES.items()):
        weights, gtype, gens = make(np.random.default_rng(1000 + ci))
        creator.create("FitPF_" + name, base.Fitness, weights=weights)
        fit = getattr(creator, "FitPF_" + name)
        if gtype == "bits":
            creator.create("IndPF_" + name, list, fitness=fit)
        else:
            creator.create("IndPF_" + name, array.array, typecode="d", fitness=fit)
        cls = getattr(creator, "IndPF_" + name)
        pf = tools.ParetoFront()
        out[name + "/weights"] = np.array(weights)
        out[name + "/gtype"] = np.array(gtype)
        for u, (genes, vals) in enumerate(gens):
            pop = []
            for row, v in zip(genes, vals):
                ind = cls(int(x) for x in row) if gtype == "bits" else cls(float(x) for x in row)
                ind.fitness.values = v
                pop.append(ind)
            pf.update(pop)
            gdt = np.uint8 if gtype == "bits" else np.float64
            key = "%s/%d/" % (name, u)
            out[key + "pop_genes"] = np.array([list(i) for i in pop], dtype=gdt)
            out[key + "pop_wv"] = np.array([i.fitness.wvalues for i in pop], dtype=np.float64)
            out[key + "front_genes"] = np.array([list(h) for h in pf], dtype=gdt)
            out[key + "front_wv"] = np.array([h.fitness.wvalues for h in pf], dtype=np.float64)
            print("%-9s update %d: pop %4d -> front %4d" % (name, u, len(pop), len(pf)))
    path = os.path.join(HERE, "pareto.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
