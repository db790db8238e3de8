import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a ROCm GPU (MI355X) and libdeapmi.so")


def golden(name):
    """A fixture archive.  One that make_golden.py wrote in pieces (NAME.npz,
    NAME.1.npz, ...: no committed file above 1 MiB) comes back whole, as a
    dict: the members of every piece, and an array stored as blocks of rows
    (``key@0``, ``key@1``, ...) joined again."""
    stem = os.path.join(GOLDEN, name[:-len(".npz")])
    paths = [stem + ".npz"]
    while os.path.exists("%s.%d.npz" % (stem, len(paths))):
        paths.append("%s.%d.npz" % (stem, len(paths)))
    if len(paths) == 1:
        return np.load(paths[0], allow_pickle=False)
    d = {}
    for p in paths:
        with np.load(p, allow_pickle=False) as z:
            d.update((k, z[k]) for k in z.files)
    for first in sorted(k for k in d if k.endswith("@0")):
        key, blocks = first[:-2], []
        while "%s@%d" % (key, len(blocks)) in d:
            blocks.append(d.pop("%s@%d" % (key, len(blocks))))
        d[key] = np.concatenate(blocks)
    return d


@pytest.fixture(scope="session")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deap_amd import _lib
    _lib.load()  # must exist on a GPU box: no fallback
    return torch.device("cuda", 0)
