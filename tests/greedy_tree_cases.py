"""Named cases for the strongest-coupling tree of the greedy solver (ASP-GREEDY-1 steps 1-3, DESIGN.md
§4.8) and a plain-Python restatement of the law with named WRONG variants beside it — shared by
tests/test_greedy_tree_cases.py (no GPU: restatement against the host tree and the CPU oracle, every
variant told apart) and tests/test_gpu_greedy_tree.py (device tree against host tree)."""
import functools

import numpy as np
import scipy.sparse

FILTER_WINDOW = 256  # bonds one workgroup of k_greedy_tree filters at once (csrc/greedy_tree.hip: kTreeThreads)

# wrong variant -> what it changes
VARIANTS = {
    "ties_reversed": "bonds of equal |w| visited in reverse generation order",
    "union_attaches_i": "two clusters: the cluster of i always hangs under the cluster of j",
    "size_ge": "two clusters: root(j) is kept when size[root(j)] >= size[root(i)]",
    "strongest_bond_only": "a fresh spin takes the sign that satisfies the visited bond alone",
    "any_cluster": "a fresh spin's row sum counts assigned neighbours of ANY cluster",
    "row_reversed": "a fresh spin's row sum runs over descending columns",
    "row_pairwise": "a fresh spin's row sum is a pairwise (tree) sum",
    "field_reversed": "the per-root field sums run over descending v",
    "isolated_not_oriented": "spins no bond touches stay +1 whatever their field",
    "flip_ge": "flip from `>= 0` (of w and of the row sum; A stores no zero, so only the row sum can tell)",
}
# wrong variant -> a named case whose result it changes
TOLD_APART = {
    "ties_reversed": "ring_ties",
    "union_attaches_i": "unequal_merge_big_i",
    "size_ge": "equal_merge_ij",
    "strongest_bond_only": "fresh_sum_beats_strongest",
    "any_cluster": "fresh_two_clusters",
    "row_reversed": "sum_order",
    "row_pairwise": "sum_order",
    "field_reversed": "components_field_order",
    "isolated_not_oriented": "isolated_fields",
    "flip_ge": "cancelling_row",
}


def couplings(J):
    """A = offdiag(J + J^T) with exact zeros dropped, canonical CSR."""
    J = scipy.sparse.csr_matrix(J, dtype=np.float64)
    J.sum_duplicates()
    A = scipy.sparse.csr_matrix(J + J.T)
    A.setdiag(0.0)
    A.eliminate_zeros()
    A.sort_indices()
    return A


def bond_count(J):
    return couplings(J).nnz // 2


def _pairwise(terms):
    if len(terms) == 0:
        return 0.0
    if len(terms) == 1:
        return terms[0]
    half = len(terms) // 2
    return _pairwise(terms[:half]) + _pairwise(terms[half:])


def tree(J, h, variant=None):
    """Steps 1-3 of ASP-GREEDY-1 in plain Python: packed uint64[ceil(K/64)], bit v set <=> spin v is +1.
    `variant`: None (the law) or a key of VARIANTS."""
    assert variant is None or variant in VARIANTS
    A = couplings(J)
    K = A.shape[0]
    indptr, indices, data = A.indptr.tolist(), A.indices.tolist(), A.data.tolist()
    h = [float(v) for v in np.asarray(h, dtype=np.float64)]
    ge = variant == "flip_ge"
    positive = (lambda v: v >= 0.0) if ge else (lambda v: v > 0.0)
    # step 1: bonds in generation order, strongest first, ties keep the generation order
    bonds = [(i, indices[k], data[k]) for i in range(K) for k in range(indptr[i], indptr[i + 1]) if indices[k] > i]
    if variant == "ties_reversed":
        order = sorted(range(len(bonds)), key=lambda b: (-abs(bonds[b][2]), -b))
    else:
        order = sorted(range(len(bonds)), key=lambda b: -abs(bonds[b][2]))  # (stable)
    parent, flip, size = [-1] * K, [0] * K, [1] * K

    def find(v):
        path, sign = [], 0
        while parent[v] != v:
            path.append(v)
            sign ^= flip[v]
            v = parent[v]
        carried = sign
        for u in path:  # compression (free: it cannot change a bit)
            mine = flip[u]
            parent[u], flip[u] = v, carried
            carried ^= mine
        return v, sign

    # step 2
    for b in order:
        i, j, w = bonds[b]
        has_i, has_j = parent[i] >= 0, parent[j] >= 0
        if not has_i and not has_j:
            parent[i], parent[j], flip[j], size[i] = i, i, int(positive(w)), 2
        elif has_i != has_j:
            fresh, other = (j, i) if has_i else (i, j)
            root, other_sign = find(other)
            terms = []
            for k in range(indptr[fresh], indptr[fresh + 1]):
                n = indices[k]
                if parent[n] < 0:
                    continue
                r, sign = find(n)
                if r != root and variant != "any_cluster":
                    continue
                terms.append(-data[k] if sign else data[k])
            if variant == "row_reversed":
                terms.reverse()
            if variant == "row_pairwise":
                energy = 0.0 + _pairwise(terms)
            else:
                energy = 0.0
                for t in terms:
                    energy = energy + t
            if variant == "strongest_bond_only":
                energy = -w if other_sign else w
            parent[fresh], flip[fresh] = root, int(positive(energy))
            size[root] += 1
        else:
            (ri, si), (rj, sj) = find(i), find(j)
            if ri == rj:
                continue
            frustrated = (si == sj) == positive(w)
            keep, gone = ri, rj
            if variant == "union_attaches_i":
                keep, gone = rj, ri
            elif size[rj] >= size[ri] if variant == "size_ge" else size[rj] > size[ri]:
                keep, gone = rj, ri
            parent[gone], flip[gone] = keep, int(frustrated)
            size[keep] += size[gone]
    # step 3
    root_of, down = list(range(K)), [0] * K
    for v in range(K):
        if parent[v] >= 0:
            root_of[v], down[v] = find(v)
    field_energy = [0.0] * K
    for v in (range(K - 1, -1, -1) if variant == "field_reversed" else range(K)):
        if variant == "isolated_not_oriented" and parent[v] < 0:
            continue
        field_energy[root_of[v]] = field_energy[root_of[v]] + (-h[v] if down[v] else h[v])
    up = np.array([not (down[v] ^ (field_energy[root_of[v]] > 0.0)) for v in range(K)], dtype=bool)
    return pack(up)


def pack(up):
    up = np.asarray(up, dtype=bool)
    words = (up.shape[0] + 63) // 64
    padded = np.zeros(max(words, 1) * 64, dtype=np.uint8)
    padded[:up.shape[0]] = up
    return np.packbits(padded, bitorder="little").view(np.uint64)[:words].copy()


def host_tree(J, h):
    """asp_sa_greedy_tree_host: the host tree the device tree must equal word for word (no device)."""
    from annealing_sign_problem_amd import annealer as sa
    from annealing_sign_problem_amd import greedy

    return greedy.greedy_tree(sa.Hamiltonian(J, h), where="host")


# ---- the cases -----------------------------------------------------------------------------------------

def _from_bonds(K, bonds, h=None):
    rows = [i for i, _, _ in bonds]
    cols = [j for _, j, _ in bonds]
    vals = [w for _, _, w in bonds]
    J = scipy.sparse.coo_matrix((vals, (rows, cols)), shape=(K, K)).tocsr()  # (upper triangle: A = J + J^T)
    return J, np.zeros(K) if h is None else np.asarray(h, dtype=np.float64)


def _random_graph(K, degree, seed, ties=False, field=True):
    rng = np.random.default_rng(seed)
    n = max(1, int(degree * K / 2))
    rows, cols = rng.integers(0, K, size=n), rng.integers(0, K, size=n)
    if ties:  # every pair once, so that every |A_ij| is 1
        pairs = np.unique(np.stack([np.minimum(rows, cols), np.maximum(rows, cols)], axis=1), axis=0)
        pairs = pairs[pairs[:, 0] != pairs[:, 1]]
        rows, cols = pairs[:, 0], pairs[:, 1]
        vals = rng.choice([-1.0, 1.0], size=rows.shape[0])
    else:
        vals = rng.normal(size=n)
    J = scipy.sparse.coo_matrix((vals, (rows, cols)), shape=(K, K)).tocsr()
    return J, (rng.normal(size=K) * 0.3 if field else np.zeros(K))


def _path(num_bonds, seed):
    """A path of num_bonds + 1 spins: every bond is a survivor, whatever the sorted order."""
    rng = np.random.default_rng(seed)
    return _from_bonds(num_bonds + 1, [(v, v + 1, float(w)) for v, w in enumerate(rng.normal(size=num_bonds))])


def _hub(row, seed):
    """Spins 0 .. row-1 chained by strong bonds, the hub (last index) bonded weakly to all of them: it is
    the last spin to join, with `row` assigned neighbours of one cluster in its row."""
    rng = np.random.default_rng(seed)
    bonds = [(v, v + 1, float(10.0 + rng.random()) * float(rng.choice([-1.0, 1.0]))) for v in range(row - 1)]
    bonds += [(v, row, float(w)) for v, w in enumerate(rng.normal(size=row) * 0.5)]
    return _from_bonds(row + 1, bonds)


def _sum_order(mirrored):
    big, chain = 2.0 ** 53, -(2.0 ** 60)
    row = [-big, 1.0, 1.0, big] if mirrored else [big, 1.0, 1.0, -big]
    return _from_bonds(5, [(0, 1, chain), (1, 2, chain), (2, 3, chain)] + [(v, 4, w) for v, w in enumerate(row)])


def _complete_then_skips():
    """A complete graph on 34 spins whose strongest 33 bonds are a spanning star (561 bonds: every bond of
    the second filter window is a skip) and a far pair joined by the weakest bond, so that the tree is not
    complete before the last bond."""
    rng = np.random.default_rng(77)
    bonds = [(0, v, float(100.0 + v)) for v in range(1, 34)]
    bonds += [(u, v, float(rng.normal())) for u in range(1, 34) for v in range(u + 1, 34)]
    bonds.append((34, 35, 1e-3))
    return _from_bonds(36, bonds)


def _planted():
    from annealing_sign_problem_amd import synthetic

    J, h, _ = synthetic.planted_cluster(3000, seed=5)
    return J, h


CASES = {
    # word tails
    "k1": lambda: (scipy.sparse.csr_matrix(np.array([[0.5]])), np.array([0.3])),
    "k2": lambda: _from_bonds(2, [(0, 1, 0.75)]),
    "k63": lambda: _random_graph(63, 4, 63),
    "k64": lambda: _random_graph(64, 4, 64),
    "k65": lambda: _random_graph(65, 4, 65),
    "k130": lambda: _random_graph(130, 5, 130),
    # spins no bond touches, with positive, negative, -0.0 and +0.0 fields
    "isolated_fields": lambda: _from_bonds(6, [(0, 1, -1.0)], [0.0, 0.0, 0.5, -0.5, -0.0, 0.0]),
    "no_bonds": lambda: (scipy.sparse.csr_matrix((70, 70)), np.where(np.arange(70) % 3 == 0, 1.0, -1.0)),
    # all |w| equal: the ties are everything
    "ring_ties": lambda: _from_bonds(12, [(v, (v + 1) % 12, 1.0 if v % 3 == 0 else -1.0) for v in range(11)]
                                     + [(0, 11, 1.0)]),
    "random_ties": lambda: _random_graph(40, 5, 40, ties=True, field=False),
    "random_ties_300": lambda: _random_graph(300, 6, 41, ties=True),
    # two clusters of equal size merged by a later bond, in both orientations of the bond; unequal ones
    "equal_merge_ij": lambda: _from_bonds(4, [(0, 1, -3.0), (2, 3, -2.5), (1, 2, 1.0)]),
    "equal_merge_ji": lambda: _from_bonds(4, [(2, 3, -3.0), (0, 1, -2.5), (1, 2, 1.0)]),
    "unequal_merge_big_i": lambda: _from_bonds(5, [(0, 1, -5.0), (1, 2, -4.0), (3, 4, -3.0), (2, 3, 1.0)]),
    "unequal_merge_big_j": lambda: _from_bonds(5, [(0, 1, -3.0), (2, 3, -5.0), (3, 4, -4.0), (1, 2, 1.0)]),
    # a fresh spin with bonds into two different clusters: only the visited bond's cluster counts
    "fresh_two_clusters": lambda: _from_bonds(5, [(0, 1, -5.0), (2, 3, -4.0), (0, 4, 1.5), (2, 4, -1.0), (3, 4, -1.0)]),
    "fresh_sum_beats_strongest": lambda: _from_bonds(4, [(0, 1, -5.0), (1, 2, -4.0), (0, 3, -1.5), (1, 3, 1.0),
                                                         (2, 3, 1.0)]),
    "cancelling_row": lambda: _from_bonds(3, [(0, 1, -4.0), (0, 2, 1.0), (1, 2, -1.0)]),
    "frustrated_triangle": lambda: _from_bonds(3, [(0, 1, 1.0), (1, 2, 1.0), (0, 2, 1.0)], [0.1, -0.2, 0.05]),
    # a hub joined last, its row around the chunk of 64
    "hub_63": lambda: _hub(63, 1),
    "hub_64": lambda: _hub(64, 2),
    "hub_65": lambda: _hub(65, 3),
    "hub_300": lambda: _hub(300, 4),
    # bond counts around a wavefront and around the filter window; all of them survivors
    "bonds_63": lambda: _path(63, 11),
    "bonds_64": lambda: _path(64, 12),
    "bonds_65": lambda: _path(65, 13),
    "bonds_window_minus_1": lambda: _path(FILTER_WINDOW - 1, 14),
    "bonds_window": lambda: _path(FILTER_WINDOW, 15),
    "bonds_window_plus_1": lambda: _path(FILTER_WINDOW + 1, 16),
    # ... and a sorted order with a whole window of skips
    "window_of_skips": _complete_then_skips,
    # several components, a field whose per-cluster sum changes sign with the order of summation
    "components_field_order": lambda: _from_bonds(7, [(0, 1, -2.0), (1, 2, -1.5), (3, 4, -1.0), (4, 5, 0.5)],
                                                  [1.0, 1e16, -1e16, -1e16, 1e16, -1.0, 0.25]),
    # the sum-order cases: the law gives 0b11111 and 0b01111
    "sum_order": lambda: _sum_order(False),
    "sum_order_mirrored": lambda: _sum_order(True),
    "planted_3000": _planted,
    # beyond the forest's LDS form
    "sparse_50000": lambda: _random_graph(50000, 4, 50000),
}
EXPECTED_WORDS = {"sum_order": 0b11111, "sum_order_mirrored": 0b01111}


@functools.lru_cache(maxsize=None)
def case(name):
    """(J csr, h) of a named case, built once."""
    J, h = CASES[name]()
    return scipy.sparse.csr_matrix(J, dtype=np.float64), np.asarray(h, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The host tree of a named case (computed once, shared by the tests; do not modify)."""
    x = host_tree(*case(name))
    x.flags.writeable = False
    return x
