"""Law ASP-PA-1 restated in plain Python integers — the checker of
tests/test_population_abi.py and tests/test_gpu_population.py, never imported by the package.

Floating point ends at the weights: Python floats are IEEE doubles with one rounding per operation,
``oracle.expneg`` is the CPU restatement of the annealer's exp(-x); from ``q`` on everything is exact
integer arithmetic on Python ints.
"""
import numpy as np

import oracle

MAX_CHAINS = 65536
DRAW_WORD = 0xFFFFFFFD  # word 2 of the Philox counter: no proposal (< 2^30), start or priority (0xFFFFFFFE) has it


def weights(energies, dbeta):
    """Steps 2-3: q_r = floor(expneg(dbeta * (E_r - min E)) * 2^31), as Python ints."""
    energies = [float(e) for e in energies]
    lowest = min(energies)
    q = []
    for e in energies:
        w = oracle.expneg(float(dbeta) * (e - lowest))
        q.append(int(w * 2.0 ** 31))  # (the product is exact: a power of two; int() is floor for w >= 0)
    return q


def draw_word(seed, sweeps_done, draw):
    """Step 4: word 0 of Philox4x32-10(counter (sweeps_done, draw, 0xFFFFFFFD, 0), key seed)."""
    seed = int(seed) & (2 ** 64 - 1)
    return int(oracle.philox4x32_10([int(sweeps_done), int(draw), DRAW_WORD, 0], [seed & 0xFFFFFFFF, seed >> 32])[0])


def select(q, v):
    """Steps 3-5 from the integer weights and the random word: (source list, survivors)."""
    R = len(q)
    assert 1 <= R <= MAX_CHAINS
    prefix = [0]
    for value in q:
        prefix.append(prefix[-1] + int(value))
    T = prefix[-1]
    assert T >= 2 ** 31 and R * T <= 2 ** 63
    U = (int(v) * T) >> 32
    source, s = [], 0
    for j in range(R):
        key = j * T + U
        while not key < R * prefix[s + 1]:  # (the keys ascend: so does s)
            s += 1
        assert R * prefix[s] <= key < R * prefix[s + 1]
        source.append(s)
    return source, len(set(source))


def resample(energies, dbeta, seed, sweeps_done, draw):
    """Steps 2-5: (q uint64[R], source uint32[R], survivors)."""
    q = weights(energies, dbeta)
    source, survivors = select(q, draw_word(seed, sweeps_done, draw))
    return np.array(q, dtype=np.uint64), np.array(source, dtype=np.uint32), survivors


def gathered(state, source):
    """Step 6 on a ``Chains.state()`` dict: numpy fancy indexing of the five arrays."""
    source = np.asarray(source, dtype=np.int64)
    out = {name: np.ascontiguousarray(state[name][source])
           for name in ("x_current", "x_best", "tracked_current", "tracked_best", "accepted")}
    out["sweeps_done"] = state["sweeps_done"]
    return out
