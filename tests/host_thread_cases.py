"""Couplings at the sizes where the plan build (csrc/sa_plan.cpp) runs on several host threads
(20 000 spins and more), in the five representations that decide its route: shared by
tests/test_host_threads.py and the GPU test of the threaded general merge in tests/test_gpu_sa.py."""
import functools

import numpy as np
import scipy.sparse

FORMS = ("symmetric", "upper", "nudged", "holed", "one_sided")


@functools.lru_cache(maxsize=None)
def forms(n):
    """{name: csr}, field for n spins of mean degree 8.  `symmetric` is exactly symmetric with a
    diagonal (the short cut A = 2 offdiag(J)); `upper` its upper triangle with doubled weights (the
    same A, bit for bit); `nudged` has one mirror element moved by one ulp and `holed` one mirror
    element missing (the recipe of test_plan_layout_matches_oracle_layout); `one_sided` holds every
    coupling as J_ij or as J_ji, never both.  All but the first go through the general merge."""
    from annealing_sign_problem_amd import synthetic

    rng = np.random.default_rng(n)
    J, _, _ = synthetic.planted_cluster(n, seed=n, mean_degree=8.0)
    J = (J + scipy.sparse.diags(rng.normal(size=n))).tocsr()
    J.sort_indices()
    assert abs(J - J.T).max() == 0
    field = rng.normal(size=n) * 1e-3
    upper = (2.0 * scipy.sparse.triu(J, 1) + scipy.sparse.diags(J.diagonal())).tocsr()
    nudged = J.copy()
    k = int(np.flatnonzero(nudged.indices != np.repeat(np.arange(n), np.diff(nudged.indptr)))[5])
    nudged.data[k] = np.nextafter(nudged.data[k], np.inf)
    coo = J.tocoo()
    keep = np.ones(coo.nnz, bool)
    keep[np.flatnonzero(coo.row > coo.col)[7]] = False
    holed = scipy.sparse.csr_matrix((coo.data[keep], (coo.row[keep], coo.col[keep])), shape=(n, n))
    above = scipy.sparse.triu(J, 1).tocoo()
    turn = rng.random(above.nnz) < 0.5
    one_sided = scipy.sparse.csr_matrix((above.data, (np.where(turn, above.col, above.row),
                                                      np.where(turn, above.row, above.col))), shape=(n, n))
    one_sided = (one_sided + scipy.sparse.diags(J.diagonal())).tocsr()
    out = {"symmetric": J, "upper": upper, "nudged": nudged, "holed": holed, "one_sided": one_sided}
    for m in out.values():
        m.sum_duplicates()
        m.sort_indices()
        for array in (m.data, m.indices, m.indptr):
            array.flags.writeable = False
    off = scipy.sparse.triu(one_sided, 1) + scipy.sparse.tril(one_sided, -1)
    assert holed.nnz == J.nnz - 1 and off.nnz == above.nnz and off.multiply(off.T).nnz == 0
    field.flags.writeable = False
    return out, field
