"""``sa.greedy_solve`` (annealing_sign_problem/common.py:250) on the MI355X path:
strongest-coupling-first cluster merging on the host, strict-descent relaxation sweeps on
the GPU (``asp_sa_greedy``; specification in DESIGN.md §4.8).  ``greedy_solve_batch`` solves many
problems in one call (``asp_sa_greedy_batch``): the same results, the descents of
all problems in a few shared launches that stop on the device."""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import _lib

MAX_RELAXATION_SWEEPS = 10000
_TREE_WHERE = {"host": 0, "device": 1, "device-hbm": 2}


def tree_where(tree=None) -> int:
    """The ``where`` of ``asp_sa_set_greedy_tree`` for a ``tree`` keyword: ``"host"`` | ``"device"``
    (| ``"device-hbm"``: the forest forced into HBM, for tests and timing); ``None`` means
    ``$ASP_GREEDY_TREE`` or ``"host"``."""
    if tree is None:
        tree = os.environ.get("ASP_GREEDY_TREE") or "host"
    if tree not in _TREE_WHERE:
        raise ValueError("tree must be 'host' or 'device', not {!r}".format(tree))
    return _TREE_WHERE[tree]


def _set_tree(lib, plan, tree) -> None:
    _lib.check(lib.asp_sa_set_greedy_tree(plan, ctypes.c_int(tree_where(tree))))


def greedy_tree(hamiltonian, where: str = "device"):
    """The configuration of the strongest-coupling tree alone (no
    relaxation), packed: ``where="device"`` builds it with ``asp_sa_greedy_tree``, ``"host"`` with the
    host code the device tree must equal word for word."""
    return greedy_tree_batch([hamiltonian], where=where)[0]


def greedy_tree_batch(hamiltonians, where: str = "device"):
    """``[greedy_tree(h, where) for h in hamiltonians]``, the device trees in shared launches
    (``asp_sa_greedy_tree_batch``)."""
    lib = _lib.load()
    hamiltonians = list(hamiltonians)
    n = len(hamiltonians)
    code = tree_where(where)
    words = [(h.size + 63) // 64 for h in hamiltonians]
    xs = [np.zeros(max(w, 1), dtype=np.uint64) for w in words]
    if code == 0:
        for h, x in zip(hamiltonians, xs):
            indptr, indices, data, field = h._arrays()
            _lib.check(lib.asp_sa_greedy_tree_host(ctypes.c_uint64(h.size), _lib.ptr(indptr), _lib.ptr(indices),
                                                   _lib.ptr(data), _lib.ptr(field), _lib.ptr(x)))
        return [x[:w] for x, w in zip(xs, words)]
    if len({id(h) for h in hamiltonians}) != n:
        raise ValueError("greedy_tree_batch: every problem needs its own Hamiltonian object")
    plans = (ctypes.c_void_p * max(n, 1))()
    outs = (ctypes.c_void_p * max(n, 1))()
    for i, h in enumerate(hamiltonians):
        plans[i] = h.plan()
        outs[i] = xs[i].ctypes.data
        _lib.check(lib.asp_sa_set_greedy_tree(plans[i], ctypes.c_int(code)))
    try:
        _lib.check(lib.asp_sa_greedy_tree_batch(plans, ctypes.c_uint32(n), outs))
    finally:
        for i in range(n):
            lib.asp_sa_set_greedy_tree(plans[i], ctypes.c_int(0))
    return [x[:w] for x, w in zip(xs, words)]


def last_tree_ms():
    """``(total, bonds + sort, k_greedy_tree, orientation)`` device ms of this thread's last device trees."""
    lib = _lib.load()
    parts = [ctypes.c_float(0.0) for _ in range(3)]
    _lib.check(lib.asp_sa_greedy_tree_last_split_ms(*[ctypes.byref(p) for p in parts]))
    return (float(lib.asp_sa_greedy_tree_last_ms()),) + tuple(float(p.value) for p in parts)


def greedy_solve(hamiltonian, max_sweeps: int = MAX_RELAXATION_SWEEPS, tree=None):
    """Returns ``(x, e)``: packed configuration (uint64[ceil(K/64)]) and its energy.  ``tree``: where
    the strongest-coupling tree is built (:func:`tree_where`); the result does not depend on it."""
    lib = _lib.load()
    _set_tree(lib, hamiltonian.plan(), tree)
    words = (hamiltonian.size + 63) // 64
    x = np.zeros(max(words, 1), dtype=np.uint64)
    e = ctypes.c_double(0.0)
    sweeps = ctypes.c_uint32(0)
    energy = np.zeros(1, dtype=np.float64)
    _lib.check(lib.asp_sa_greedy(hamiltonian.plan(), ctypes.c_uint32(int(max_sweeps)), _lib.ptr(x),
                                 _lib.ptr(energy), ctypes.byref(sweeps)))
    return x[:words], float(energy[0])


def greedy_solve_batch(hamiltonians, max_sweeps: int = MAX_RELAXATION_SWEEPS, return_sweeps: bool = False,
                       tree=None):
    """``[greedy_solve(h, max_sweeps) for h in hamiltonians]`` in ONE device call: bit for bit the
    same ``(x, e)`` per problem, in input order, whatever the composition of the batch.  Every
    problem needs its own Hamiltonian object.  ``return_sweeps``: ``(x, e, t)`` instead, ``t`` the
    exact number of descent sweeps performed (the index of the first sweep that flipped nothing,
    or ``max_sweeps``).  ``tree``: as in :func:`greedy_solve`, or one value per problem."""
    lib = _lib.load()
    hamiltonians = list(hamiltonians)
    trees = list(tree) if isinstance(tree, (list, tuple)) else [tree] * len(hamiltonians)
    if len(trees) != len(hamiltonians):
        raise ValueError("greedy_solve_batch: one tree per problem")
    tree_codes = [tree_where(t) for t in trees]
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
        _lib.check(lib.asp_sa_set_greedy_tree(items[i].plan, ctypes.c_int(tree_codes[i])))
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
