"""Formulas of the batched resolution tests (csrc/resolution_batch.hip), shared
by tests/test_res_batch_gpu.py (GPU: exact against the oracle), by
tests/golden/make_golden_paths.py (the reference's own verdict of each) and by
the tests that hold the oracle and the kernel to those verdicts."""
import functools
import random

EDGE = [[], [[]], [[1]], [[1], [-1]], [[1, -1]], [[1, 1], [-1]], [[1, 2], [], [-1]], [[1, -1], [1, -1]]]


@functools.lru_cache(maxsize=None)
def mix():
    """200 formulas drawn as test_resolution_gpu.py::test_matches_oracle_random draws its 60."""
    rng = random.Random(17)
    fs = []
    for it in range(200):
        n = rng.randint(2, 7)
        m = rng.randint(1, 12)
        f = [[v if rng.random() < 0.5 else -v for v in rng.sample(range(1, n + 1), rng.randint(1, min(3, n)))]
             for _ in range(m)]
        if it % 7 == 0:
            f.append(list(f[0]))                      # duplicate clause
        if it % 11 == 0:
            f.append([1, -1, 2][:min(3, n + 1)])      # tautological input clause
        fs.append(f)
    return fs
