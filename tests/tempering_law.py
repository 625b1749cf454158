"""Law ASP-PT-1 restated in plain Python — the checker of tests/test_tempering_abi.py
and tests/test_gpu_tempering.py, never imported by the package.

Python floats are IEEE doubles with one rounding per operation, ``oracle.expneg`` is the CPU restatement
of the annealer's exp(-x) and ``oracle.philox4x32_10`` of its random words.  The device decides a
proposal through ``metropolis_accept_word``, a filter whose result always equals ``u < expneg(x)`` with
``u = (word + 0.5) 2^-32`` and ``expneg(x) = 0`` for every ``x`` that is not below 23 (csrc/sa_device.hpp);
that is what is restated here.
"""
import numpy as np

import oracle

DRAW_WORD = 0xFFFFFFFC  # word 2 of the Philox counter: proposals and starts have < 2^30 there, the
                        # priorities 0xFFFFFFFE, the resampling 0xFFFFFFFD


def pairs(R, parity):
    """Step 2: the k of the pairs (k, k + 1)."""
    assert parity in (0, 1)
    return [k for k in range(parity, R - 1, 2)]


def cost(beta_k, beta_k1, e_k, e_k1):
    """Step 3: x_k = (beta_{k+1} - beta_k) * (E_k - E_{k+1}), one rounding per operation."""
    return (float(beta_k1) - float(beta_k)) * (float(e_k) - float(e_k1))


def threshold(x):
    """The probability that a pair of cost x swaps: 1 for x <= 0, else expneg(x) (0 from 23 on)."""
    if x <= 0.0:
        return 1.0
    return oracle.expneg(x) if x < 23.0 else 0.0


def draw_word(seed, k, sweeps_done, draw):
    """Step 4: word 0 of Philox4x32-10(counter (k, sweeps_done, 0xFFFFFFFC, draw), key seed)."""
    seed = int(seed) & (2 ** 64 - 1)
    return int(oracle.philox4x32_10([int(k), int(sweeps_done), DRAW_WORD, int(draw)],
                                    [seed & 0xFFFFFFFF, seed >> 32])[0])


def accepts(v, x):
    """Step 4: x <= 0, or u < expneg(x) with x < 23 for u = (v + 0.5) 2^-32."""
    if x <= 0.0:
        return True
    if not x < 23.0:  # (also a cost that is not a number)
        return False
    return (float(int(v)) + 0.5) * 2.0 ** -32 < oracle.expneg(x)


def select(energies, betas, parity, words):
    """Steps 2-5 with the random word of pair k given as words[k]: (source list, accepted)."""
    R = len(energies)
    assert len(betas) == R
    source, accepted = list(range(R)), 0
    for k in pairs(R, parity):
        if accepts(words[k], cost(betas[k], betas[k + 1], energies[k], energies[k + 1])):
            source[k], source[k + 1] = k + 1, k
            accepted += 1
    return source, accepted


def exchange(energies, betas, parity, seed, sweeps_done, draw):
    """Steps 2-5: (source uint32[R], accepted)."""
    words = {k: draw_word(seed, k, sweeps_done, draw) for k in pairs(len(energies), parity)}
    source, accepted = select(energies, betas, parity, words)
    return np.array(source, dtype=np.uint32), accepted
