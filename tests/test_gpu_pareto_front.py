"""tools.ParetoFront on the device: ``update(DevicePopulation)`` (one
dm_pareto_update per call) against the reference's ParetoFront
(tests/golden/pareto.npz), against the class's own host loop, through the C ABI
directly, mixed with host edits, and inside the drivers."""
import ctypes

import numpy as np
import pytest

from conftest import golden
from test_pareto_front import CASES, front_arrays, host_individuals, same_bits

pytestmark = pytest.mark.gpu


def _dp():
    from deap_amd.device import DevicePopulation
    return DevicePopulation


@pytest.fixture(scope="module")
def fx():
    return golden("pareto.npz")


def _device_pop(genes, wv, weights, gtype):
    return _dp().from_numpy(genes, weights=weights, gtype=gtype, wvalues=wv,
                            valid=np.ones(len(genes)))


def _fronts_equal(a, b):
    return ([list(h) for h in a] == [list(h) for h in b] and
            [h.fitness.wvalues for h in a] == [h.fitness.wvalues for h in b])


@pytest.mark.parametrize("case", CASES)
def test_fixture_replay_on_device(gpu, fx, case, monkeypatch):
    from deap_amd import tools
    weights = tuple(fx[case + "/weights"].tolist())
    gtype = str(fx[case + "/gtype"])
    pf = tools.ParetoFront()
    for u in range(4):
        key = "%s/%d/" % (case, u)
        pg, pw = fx[key + "pop_genes"], fx[key + "pop_wv"]
        pf.update(_device_pop(pg, pw, weights, gtype))
        assert pf._dev_ok  # the closed form ran, not the host loop
        # the length comes without a row fetch
        with monkeypatch.context() as mp:
            mp.setattr(_dp(), "to_individuals", None)
            assert len(pf) == len(fx[key + "front_wv"]), (case, u)
        genes, wv = front_arrays(pf, pg.dtype, pg.shape[1], len(weights))
        assert same_bits(wv, fx[key + "front_wv"]), (case, u)
        assert same_bits(genes, fx[key + "front_genes"]), (case, u)
    dev = pf.front()
    g, w, ok = dev.to_numpy()
    assert ok.all() and same_bits(w, fx[case + "/3/front_wv"])
    assert same_bits(g.astype(fx[case + "/3/front_genes"].dtype), fx[case + "/3/front_genes"])


def _abi(ctx, archive, pop, out, cap, src):
    from deap_amd import _lib
    n_out = ctypes.c_int64(-1)
    c_out = out.c_pop(0, 0)
    rc = _lib.load().dm_pareto_update(
        ctx, ctypes.byref(archive), ctypes.byref(pop), ctypes.byref(c_out), cap,
        ctypes.byref(n_out), ctypes.c_void_p(src.data_ptr()) if src is not None else None)
    return rc, n_out.value


def test_direct_abi(gpu, fx):
    import torch
    from deap_amd import _lib
    weights = tuple(fx["wide2/weights"].tolist())
    p0 = _device_pop(fx["wide2/0/pop_genes"], fx["wide2/0/pop_wv"], weights, "f64")
    p1 = _device_pop(fx["wide2/1/pop_genes"], fx["wide2/1/pop_wv"], weights, "f64")
    ctx = p0.ctx.bind()
    a = p0.like(0, capacity=2048)
    b = p0.like(0, capacity=2048)
    src = torch.empty(2048, dtype=torch.int32, device=gpu)

    # an empty archive
    rc, n = _abi(ctx, a.c_pop(0, 0), p0.c_pop(), b, 2048, src)
    assert rc == _lib.DM_OK and n == 300
    b.resize(n)
    s = src[:n].cpu().numpy()
    assert (s < 0).all() and sorted(-s - 1) == list(range(300))
    assert same_bits(b.genes_numpy(), fx["wide2/0/pop_genes"][-s - 1])
    assert same_bits(b.wvalues[:n].cpu().numpy(), fx["wide2/0/front_wv"])

    # archive + population: src names the rows the output rows came from
    rc, n = _abi(ctx, b.c_pop(), p1.c_pop(), a, 2048, src)
    assert rc == _lib.DM_OK and n == len(fx["wide2/1/front_wv"])
    a.resize(n)
    s = src[:n].cpu().numpy()
    old, new = b.genes_numpy(), fx["wide2/1/pop_genes"]
    assert (s >= 0).any() and (s < 0).any() and s.max() < 300 and s.min() >= -513
    want = np.array([old[i] if i >= 0 else new[-i - 1] for i in s])
    assert same_bits(a.genes_numpy(), want)
    assert same_bits(a.genes_numpy(), fx["wide2/1/front_genes"])
    assert a.valid[:n].cpu().numpy().all()

    # an empty population returns the archive unchanged
    rc, n2 = _abi(ctx, a.c_pop(), p1.c_pop(0, 0), b, 2048, src)
    assert rc == _lib.DM_OK and n2 == n
    b.resize(n2)
    assert same_bits(b.genes_numpy(), a.genes_numpy())
    assert same_bits(b.wvalues[:n].cpu().numpy(), a.wvalues[:n].cpu().numpy())
    assert src[:n].cpu().numpy().tolist() == list(range(n))

    # capacity one short, and an aliased out
    rc, _ = _abi(ctx, a.c_pop(), p1.c_pop(), b, n + 513 - 1, None)
    assert rc == _lib.DM_ERR_INVALID and "out_capacity" in _lib.last_error()
    rc, _ = _abi(ctx, a.c_pop(), p1.c_pop(), a, 2048, None)
    assert rc == _lib.DM_ERR_INVALID and "alias" in _lib.last_error()
    rc, _ = _abi(ctx, a.c_pop(), p1.c_pop(), p1, 2048, None)
    assert rc == _lib.DM_ERR_INVALID


def _tie_population(rng, n, nobj, dim):
    genes = rng.uniform(-1, 1, (n, dim))
    wv = np.round(rng.uniform(0, 1, (n, nobj)), 2)
    dup = rng.choice(n, n // 5, replace=False)
    from_ = rng.integers(0, n, n // 5)
    genes[dup], wv[dup] = genes[from_], wv[from_]
    return genes, wv


def test_random_ties_equal_host_loop(gpu):
    """n = 5,000, 3 objectives rounded to two decimals, a fifth of the rows
    exact copies: the device front equals the class's own host loop over the
    same rows, three updates in a row."""
    from deap_amd import tools
    rng = np.random.default_rng(11)
    weights = (1.0, -1.0, 1.0)
    dev, host = tools.ParetoFront(), tools.ParetoFront()
    for _ in range(3):
        genes, wv = _tie_population(rng, 5000, 3, 8)
        dev.update(_device_pop(genes, wv, weights, "f64"))
        host.update(host_individuals(genes, wv, weights))
        assert dev._dev_ok
        # neither trivial nor slow: 25, 32 and 36 rows with these draws (the
        # maxima of 5,000 uniform points in a cube number about ln(n)^2 / 2)
        assert 10 < len(host) < 1000
        assert len(dev) == len(host)
        assert _fronts_equal(dev, host)


def test_f32_genomes_equal_host_loop(gpu):
    """fp32 rows (their own hash and equality path), an odd dimension, zeros
    of both signs and NaN genes among few distinct genomes."""
    from deap_amd import tools
    rng = np.random.default_rng(3)
    weights = (1.0, -1.0)
    pool = rng.integers(-1, 2, (12, 7)).astype(np.float32)
    pool[3, 2], pool[4, 2] = 0.0, -0.0
    pool[4, [0, 1, 3, 4, 5, 6]] = pool[3, [0, 1, 3, 4, 5, 6]]  # equal but for the zero's sign
    pool[5, 6] = np.nan
    dev, host = tools.ParetoFront(), tools.ParetoFront()
    for n in (300, 700):
        pick = rng.integers(0, 12, n)
        a = rng.integers(0, 6, n)
        wv = np.stack([a, 5 - a - rng.integers(0, 2, n)], 1).astype(np.float64)
        pop = _dp().from_numpy(pool[pick], weights=weights, gtype="f32", wvalues=wv,
                               valid=np.ones(n))
        dev.update(pop)
        host.update(pop.to_individuals())
        assert dev._dev_ok and len(dev) == len(host)
        assert repr([(list(h), h.fitness.wvalues) for h in dev]) == \
            repr([(list(h), h.fitness.wvalues) for h in host])
    kept = [list(h) for h in dev]
    assert sum(1 for g in kept if g[6] != g[6]) > 2      # NaN rows are nobody's twin
    assert len(kept) > len({repr(g) for g in kept})


@pytest.mark.parametrize("bad", ["invalid", "nan"])
def test_outside_the_closed_form_equals_host_path(gpu, bad):
    """An invalid row or a NaN wvalue: the device call declines and the host
    loop runs over the materialised population."""
    from deap_amd import tools
    rng = np.random.default_rng(5)
    weights = (1.0, 1.0)
    genes = rng.integers(0, 3, (40, 4)).astype(np.float64)
    wv = rng.integers(0, 4, (40, 2)).astype(np.float64)
    valid = np.ones(40)
    if bad == "invalid":
        valid[7] = 0
    else:
        wv[7, 1] = np.nan
    dev, host = tools.ParetoFront(), tools.ParetoFront()
    first = _device_pop(genes[:20], wv[:20], weights, "f64")
    dev.update(first)
    host.update(first.to_individuals())
    pop = _dp().from_numpy(genes, weights=weights, gtype="f64", wvalues=wv, valid=valid)
    dev.update(pop)
    assert not dev._dev_ok
    host.update(pop.to_individuals())
    assert len(dev) == len(host)
    # (through repr: a NaN wvalue is not == itself)
    assert repr([(list(h), h.fitness.wvalues) for h in dev]) == \
        repr([(list(h), h.fitness.wvalues) for h in host])


def test_mixed_host_and_device_use(gpu, fx):
    from deap_amd import tools
    weights = tuple(fx["lattice3/weights"].tolist())
    dev, host = tools.ParetoFront(), tools.ParetoFront()

    def both(u, device=True):
        pg, pw = fx["lattice3/%d/pop_genes" % u], fx["lattice3/%d/pop_wv" % u]
        dev.update(_device_pop(pg, pw, weights, "bits"))
        host.update(host_individuals(pg, pw, weights))
        assert dev._dev_ok == device
        assert len(dev) == len(host) and _fronts_equal(dev, host)

    both(2)
    # a new genome under the best entry's fitness: the hall stays a front
    peer = host_individuals(1 - fx["lattice3/3/pop_genes"][:1], [host[0].fitness.wvalues],
                            weights)[0]
    for pf in (dev, host):
        pf.insert(peer)
    assert not dev._dev_ok and len(dev) == len(host) and list(dev[0]) == list(peer)
    both(3)
    for pf in (dev, host):
        pf.remove(0)
        pf.remove(-1)
    both(1)
    # an entry that dominates the others: insert() does not evict them
    # (support.py:550-560), the hall is no front any more and the update
    # takes the reference's loop until it is one again
    ideal = host_individuals(fx["lattice3/3/pop_genes"][:1], np.array([[-0.0, 2.0, -0.0]]),
                             weights)[0]
    n = len(host)
    for pf in (dev, host):
        pf.insert(ideal)
    both(3, device=False)
    assert len(dev) == n + 1
    for pf in (dev, host):
        pf.clear()
    assert len(dev) == 0 and list(dev) == []
    both(1)
    both(2)
    assert len(dev.front()) == len(host)


class _Recorder:
    """A hall that sees what the drivers hand it and keeps a host-only
    ParetoFront of it; no update_begin, so every driver calls update."""

    def __init__(self):
        from deap_amd import tools
        self.front = tools.ParetoFront()

    def update(self, population):
        self.front.update(population.to_individuals())


def _zdt1_run(hall, driver):
    from deap_amd import algorithms, base, benchmarks, tools
    from deap_amd.ops import RandomStream
    stream = RandomStream(21)
    pop = tools.initPopulation(n=64, dim=30, low=0.2, high=0.8, gtype="f64",
                               weights=(-1.0, -1.0), stream=stream)
    tb = base.Toolbox()
    tb.register("evaluate", benchmarks.zdt1)
    tb.register("mate", tools.cxBlend, alpha=0.1)
    tb.register("mutate", tools.mutGaussian, mu=0, sigma=0.01, indpb=0.1)
    if driver == "simple":
        tb.register("select", tools.selTournament, tournsize=3)
        benchmarks.zdt1(pop)
        pop, _ = algorithms.eaSimple(pop, tb, 0.6, 0.3, 5, halloffame=hall, verbose=False,
                                     stream=stream)
    else:
        tb.register("select", tools.selNSGA2)
        drv = algorithms.eaMuPlusLambda if driver == "plus" else algorithms.eaMuCommaLambda
        pop, _ = drv(pop, tb, 64, 128, 0.6, 0.3, 5, halloffame=hall, verbose=False,
                     stream=stream)
    return pop.to_numpy()


@pytest.mark.parametrize("driver", ["plus", "comma", "simple"])
def test_drivers_accept_a_pareto_front(gpu, driver):
    """ZDT1, dim 30, five generations with halloffame=ParetoFront(): the same
    front as a host-only ParetoFront fed the same populations, and the run
    itself bit-identical (the hall does not disturb it)."""
    from deap_amd import tools
    pf, rec = tools.ParetoFront(), _Recorder()
    g1, w1, ok1 = _zdt1_run(pf, driver)
    g2, w2, ok2 = _zdt1_run(rec, driver)
    assert same_bits(g1, g2) and same_bits(w1, w2) and np.array_equal(ok1, ok2)
    assert not np.isnan(w1).any() and pf._dev_ok  # the device path all the way
    assert len(pf) == len(rec.front) and len(pf) > 1
    assert _fronts_equal(pf, rec.front)


def test_checkpoint_round_trip_on_device(gpu, fx, tmp_path):
    from deap_amd import checkpoint, tools
    weights = tuple(fx["lattice2/weights"].tolist())
    pf = tools.ParetoFront()
    for u in range(3):
        pop = _device_pop(fx["lattice2/%d/pop_genes" % u], fx["lattice2/%d/pop_wv" % u], weights,
                          "f64")
        pf.update(pop)
    path = str(tmp_path / "ck.npz")
    checkpoint.save(path, pop, halloffame=pf)
    back = checkpoint.load(path)["halloffame"]
    assert type(back) is tools.ParetoFront and _fronts_equal(back, pf)
    nxt = _device_pop(fx["lattice2/3/pop_genes"], fx["lattice2/3/pop_wv"], weights, "f64")
    back.update(nxt)
    assert same_bits(front_arrays(back, np.float64, 5, 2)[1], fx["lattice2/3/front_wv"])
