"""``bench.py --dump-outputs DIR`` and the plain / ``--full`` split.

A plain run times the steps and prints the headline line only; ``--full``
adds the CPU baseline, the deme digests and C5's stage breakdown.
``--dump-outputs`` writes what the last timed step left as float32 / float64
``.npy`` files, at most 64 MB in all, bit-identical from run to run for the
same arguments (seeded Philox streams, a fixed seeded row sample).  The runs
are in-process (``bench.main``) at small populations: c3 above and the others
below the 4,096 pairs from which the generation kernel orders its pairs."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps")


def _run(capsys, args):
    import bench
    capsys.readouterr()
    assert not bench.main(args)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _load(d):
    return {f: np.load(os.path.join(d, f), allow_pickle=False) for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("cfg,pop", [("c3", 8197), ("c2", 4099), ("c3f32", 1000), ("zdt1", 1000),
                                     ("c5", 4096), ("c5x", 4096)])
def test_dump_outputs_is_reproducible(gpu, capsys, tmp_path, cfg, pop):
    common = ["--gpus", "1", "--config", cfg, "--pop", str(pop), "--steps", "3", "--warmup", "1",
              "--warmup-secs", "0"]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    one = _run(capsys, common + ["--dump-outputs", a])
    two = _run(capsys, common + ["--dump-outputs", b])
    for k in HEADLINE:
        assert k in one, k
    assert one["steps"] == 3 and one["ms_per_step"] > 0 and one["higher_is_better"] is True
    # value = individuals x steps / the timed seconds, ms_per_step = those seconds / steps
    # (printed with four decimals)
    assert abs(pop / one["value"] * 1e3 - one["ms_per_step"]) <= 1e-4
    # a plain run does the headline's work only
    assert one["cpu_baseline"] is None and "deme_digests" not in one
    assert "selection" not in one and "count_pass" not in one
    fa, fb = _load(a), _load(b)
    assert fa and sorted(fa) == sorted(fb)
    assert sum(os.path.getsize(os.path.join(a, f)) for f in fa) <= 64e6
    for f, x in fa.items():
        assert f.endswith(".npy") and x.dtype in (np.float32, np.float64), f
        assert x.tobytes() == fb[f].tobytes(), f
    name = "replica0" if cfg in ("c5", "c5x") else "deme0"
    rows = fa[name + "_rows.npy"].astype(np.int64)
    dim = {"c3": 1000, "c2": 4096, "c3f32": 1000, "zdt1": 30, "c5": 12, "c5x": 12}[cfg]
    assert fa[name + "_genes.npy"].shape == (len(rows), dim)
    assert len(fa[name + "_wvalues_all.npy"]) == pop
    assert np.array_equal(fa[name + "_wvalues.npy"], fa[name + "_wvalues_all.npy"][rows],
                          equal_nan=True)
    assert np.all(fa[name + "_valid_all.npy"] == 1.0)
    if cfg == "c2":  # OneMax: the dumped fitness is the dumped genome's bit count
        assert np.array_equal(fa[name + "_genes.npy"].sum(axis=1), fa[name + "_wvalues.npy"][:, 0])


def test_sampled_rows_are_a_fixed_choice(gpu, capsys, tmp_path, monkeypatch):
    """A population larger than its share of the dump is sampled: the same
    sorted rows every run, the whole fitness beside them."""
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 20)
    args = ["--gpus", "1", "--pop", "1500", "--steps", "2", "--warmup", "0", "--warmup-secs", "0"]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _run(capsys, args + ["--dump-outputs", a])
    _run(capsys, args + ["--dump-outputs", b])
    fa, fb = _load(a), _load(b)
    rows = fa["deme0_rows.npy"]
    assert 0 < len(rows) < 1500 and np.all(np.diff(rows) > 0)
    assert sum(os.path.getsize(os.path.join(a, f)) for f in fa) <= 1 << 20
    for f in fa:
        assert fa[f].tobytes() == fb[f].tobytes(), f
    assert fa["deme0_nevals.npy"].shape == (1,) and 0 < fa["deme0_nevals.npy"][0] <= 1500


def test_full_adds_the_checks(gpu, capsys, tmp_path):
    """``--full`` reports the digests (a different --steps gives another
    population, so --steps does set the timed steps) and keeps the sanity
    checks; the dump works beside it."""
    args = ["--gpus", "1", "--pop", "2048", "--warmup", "1", "--warmup-secs", "0", "--full",
            "--no-cpu-baseline"]
    d = str(tmp_path / "d")
    three = _run(capsys, args + ["--steps", "3", "--dump-outputs", d])
    again = _run(capsys, args + ["--steps", "3"])
    four = _run(capsys, args + ["--steps", "4"])
    assert three["deme_digests"]["check"] in ("match", "no reference")
    assert three["deme_digests"]["digest"] == again["deme_digests"]["digest"]
    assert three["deme_digests"]["digest"] != four["deme_digests"]["digest"]
    assert three["deme_digests"]["after_generation"] == 4 and four["steps"] == 4
    assert np.all(np.isfinite(_load(d)["deme0_wvalues_all.npy"]))
