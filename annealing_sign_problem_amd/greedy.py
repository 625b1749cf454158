"""``sa.greedy_solve`` (annealing_sign_problem/common.py:250) on the MI355X path:
strongest-coupling-first cluster merging on the host, strict-descent relaxation sweeps on
the GPU (``asp_sa_greedy``; specification in DESIGN.md §4.8).  ``greedy_solve_batch`` solves many
problems in one call (``asp_sa_greedy_batch``): the same results, the descents of
all problems in a few shared launches that stop on the device."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

MAX_RELAXATION_SWEEPS = 10000


def greedy_solve(hamiltonian, max_sweeps: int = MAX_RELAXATION_SWEEPS):
    """Returns ``(x, e)``: packed configuration (uint64[ceil(K/64)]) and its energy."""
    lib = _lib.load()
    words = (hamiltonian.size + 63) // 64
    x = np.zeros(max(words, 1), dtype=np.uint64)
    e = ctypes.c_double(0.0)
    sweeps = ctypes.c_uint32(0)
    energy = np.zeros(1, dtype=np.float64)
    _lib.check(lib.asp_sa_greedy(hamiltonian.plan(), ctypes.c_uint32(int(max_sweeps)), _lib.ptr(x),
                                 _lib.ptr(energy), ctypes.byref(sweeps)))
    return x[:words], float(energy[0])


def greedy_solve_batch(hamiltonians, max_sweeps: int = MAX_RELAXATION_SWEEPS, return_sweeps: bool = False):
    """``[greedy_solve(h, max_sweeps) for h in hamiltonians]`` in ONE device call: bit for bit the
    same ``(x, e)`` per problem, in input order, whatever the composition of the batch.  Every
    problem needs its own Hamiltonian object.  ``return_sweeps``: ``(x, e, t)`` instead, ``t`` the
    exact number of descent sweeps performed (the index of the first sweep that flipped nothing,
    or ``max_sweeps``)."""
    lib = _lib.load()
    hamiltonians = list(hamiltonians)
    n = len(hamiltonians)
    if len({id(h) for h in hamiltonians}) != n:
        raise ValueError("greedy_solve_batch: every problem needs its own Hamiltonian object")
    items = (_lib.SaGreedyItem * max(n, 1))()
    xs, words = [], []
    energies = np.zeros(max(n, 1), dtype=np.float64)
    sweeps = np.zeros(max(n, 1), dtype=np.uint32)
    for i, h in enumerate(hamiltonians):
        words.append((h.size + 63) // 64)
        xs.append(np.zeros(max(words[i], 1), dtype=np.uint64))
        items[i].plan = h.plan()
        items[i].max_sweeps = int(max_sweeps)
        items[i].flags = 0
        items[i].out_x = xs[i].ctypes.data
        items[i].out_e = energies.ctypes.data + 8 * i
        items[i].out_sweeps = sweeps.ctypes.data + 4 * i if return_sweeps else None
    _lib.check(lib.asp_sa_greedy_batch(items, ctypes.c_uint32(n)))
    if return_sweeps:
        return [(xs[i][:words[i]], float(energies[i]), int(sweeps[i])) for i in range(n)]
    return [(xs[i][:words[i]], float(energies[i])) for i in range(n)]


def last_batch_ms():
    """``(host tree ms, device descent ms)`` of this thread's last :func:`greedy_solve_batch`."""
    tree, descent = ctypes.c_float(0.0), ctypes.c_float(0.0)
    _lib.check(_lib.load().asp_sa_greedy_batch_last_ms(ctypes.byref(tree), ctypes.byref(descent)))
    return float(tree.value), float(descent.value)
