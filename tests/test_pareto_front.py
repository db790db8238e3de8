"""tools.ParetoFront on the host (no GPU): the class's own loop
(``update(list of individuals)``) against the reference's ParetoFront
(tests/golden/pareto.npz, written by tests/golden/make_golden_pareto.py),
pickling, the checkpoint helpers and the export."""
import pickle

import numpy as np
import pytest

from conftest import golden

CASES = ("lattice2", "lattice3", "wide2", "single", "nan_gene")


class Ind(list):
    pass


def host_individuals(genes, wv, weights):
    """Fresh host individuals (lists with a HostFitness) from fixture rows."""
    from deap_amd.device import HostFitness
    out = []
    for g, w in zip(genes, wv):
        ind = Ind(g.tolist())
        ind.fitness = HostFitness(weights)
        ind.fitness.wvalues = tuple(float(x) for x in w)
        out.append(ind)
    return out


def front_arrays(pf, gdtype, dim, nobj):
    genes = np.array([list(h) for h in pf], dtype=gdtype).reshape(len(pf), dim)
    wv = np.array([h.fitness.wvalues for h in pf], dtype=np.float64).reshape(len(pf), nobj)
    return genes, wv


def same_bits(a, b):
    """Exact equality, NaN payloads and the sign of zero included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def fx():
    return golden("pareto.npz")


@pytest.mark.parametrize("case", CASES)
def test_host_update_reproduces_the_reference(fx, case):
    from deap_amd import tools
    weights = tuple(fx[case + "/weights"].tolist())
    pf = tools.ParetoFront()
    for u in range(4):
        key = "%s/%d/" % (case, u)
        pg, pw = fx[key + "pop_genes"], fx[key + "pop_wv"]
        pf.update(host_individuals(pg, pw, weights))
        genes, wv = front_arrays(pf, pg.dtype, pg.shape[1], len(weights))
        assert len(pf) == len(fx[key + "front_wv"])
        assert same_bits(wv, fx[key + "front_wv"]), (case, u)
        assert same_bits(genes, fx[key + "front_genes"]), (case, u)
        # keys mirror items, ascending (support.py:550-560)
        assert [k.wvalues for k in pf.keys] == [h.fitness.wvalues for h in reversed(pf)]


def test_fixture_forces_what_it_claims(fx):
    # the archive crosses the 256-row tile of the cross kernel
    assert len(fx["wide2/0/front_wv"]) == 300 and len(fx["wide2/1/front_wv"]) > 256
    # zeros of both signs among the lattice fitnesses
    w = np.concatenate([fx["lattice2/%d/pop_wv" % u] for u in range(4)])
    assert (np.signbit(w) & (w == 0)).any() and (~np.signbit(w) & (w == 0)).any()
    # the NaN rows all stay: two per population of more than one row
    g = fx["nan_gene/3/front_genes"]
    assert np.isnan(g).any(axis=1).sum() == 6
    # one objective: a single equal-fitness run
    assert len(np.unique(fx["single/3/front_wv"])) == 1 and len(fx["single/3/front_wv"]) > 5


def test_exported_and_unbounded():
    from deap_amd import tools
    assert "ParetoFront" in tools.__all__
    pf = tools.ParetoFront()
    assert isinstance(pf, tools.HallOfFame) and pf.maxsize is None and len(pf) == 0
    # the drivers take update() when a hall has no update_begin
    assert getattr(pf, "update_begin", None) is None


def _small_front(fx):
    from deap_amd import tools
    weights = tuple(fx["lattice2/weights"].tolist())
    pf = tools.ParetoFront()
    for u in range(3):
        pf.update(host_individuals(fx["lattice2/%d/pop_genes" % u], fx["lattice2/%d/pop_wv" % u],
                                   weights))
    return pf


def test_container_interface(fx):
    pf = _small_front(fx)
    n = len(pf)
    assert n == len(fx["lattice2/2/front_wv"]) and n > 3
    assert pf[0] is pf.items[0] and pf[-1] is pf.items[-1] and pf[1:3] == pf.items[1:3]
    assert list(reversed(pf)) == list(pf)[::-1]
    assert str(pf) == str(pf.items)
    best = pf[0]
    pf.remove(0)
    assert len(pf) == n - 1 and len(pf.keys) == n - 1 and pf[0] is not best
    pf.insert(best)
    assert len(pf) == n and list(pf[0]) == list(best) and pf[0] is not best  # a deep copy
    pf.clear()
    assert len(pf) == 0 and pf.keys == [] and pf.items == []


def test_pickle_round_trip(fx):
    pf = _small_front(fx)
    back = pickle.loads(pickle.dumps(pf))
    assert type(back) is type(pf) and back.maxsize is None and back.similar is pf.similar
    assert [list(h) for h in back] == [list(h) for h in pf]
    assert [h.fitness.wvalues for h in back] == [h.fitness.wvalues for h in pf]
    # the copy keeps working
    weights = tuple(fx["lattice2/weights"].tolist())
    pop = host_individuals(fx["lattice2/3/pop_genes"], fx["lattice2/3/pop_wv"], weights)
    back.update(pop)
    assert same_bits(front_arrays(back, np.float64, 5, 2)[1], fx["lattice2/3/front_wv"])


def test_checkpoint_keeps_the_class(fx):
    from deap_amd import checkpoint, tools
    pf = _small_front(fx)

    class Meta:  # header() reads the population's layout only
        dim, gtype, weights, stride = 5, 2, (1.0, 1.0), 64

        def __len__(self):
            return 0
    h = checkpoint.header(Meta(), halloffame=pf)
    assert h["halloffame"]["maxsize"] is None
    assert len(h["halloffame"]["items"]) == len(pf)
    hof, _ = checkpoint.to_reference_types(pf, None, tools)
    assert type(hof) is tools.ParetoFront
    assert [list(x) for x in hof] == [list(x) for x in pf]
    assert [x.fitness.wvalues for x in hof] == [x.fitness.wvalues for x in pf]
    bounded = tools.HallOfFame(3)
    assert type(checkpoint.to_reference_types(bounded, None, tools)[0]) is tools.HallOfFame
